// phj_capi.hip — the C ABI (include/phj.h) over the gfx950 kernels.
//
// Orchestration of the reference's HashJoiner::Run on one MI355X:
//   radix:          Partition(R), Partition(S)            RadixCluster/HashJoin.hpp:208-224
//                   -> build + probe per partition        :243-331
//   no-partitioning: Build(R) -> Probe(S)                 NoPartitioning/HashJoin.hpp:54-187
// Every kernel is launched on the ctx stream; device buffers are allocated
// once (grow-only) before the timed region; phases are timed with hipEvents
// on the same stream. Errors never cross the ABI as exceptions: they become
// negative status codes plus a message (phj_last_error).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <functional>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <vector>

// Measurement builds only (scripts/ab_lib.sh, `make prof-lib`): the phase-clock
// forms of S's pass 1 and of the LDS join's builds, printed to stderr per join.
// 0: an A/B build without the hot-key pre-aggregation (phj_hot.h; scripts/ab_lib.sh)
#ifndef PHJ_PREAGG
#define PHJ_PREAGG 1
#endif
// With the hot-key pre-aggregation, R's chain runs on the aux stream beside
// the hot-key prologue, on all but PHJ_HOT_FREE_CUS CUs per shard of its pass 1
#ifndef PHJ_HOT_FREE_CUS
#define PHJ_HOT_FREE_CUS 6
#endif
#ifndef PHJ_P1_PROF
#define PHJ_P1_PROF 0
#endif
#ifndef PHJ_CL_PROF
#define PHJ_CL_PROF 0
#endif

#include "../../include/phj.h"
#include "phj_cluster.h"
#include "phj_join.h"
#include "phj_inner.h"
#include "phj_outer.h"
#include "phj_index.h"
#include "phj_ordinal.h"
#include "phj_agg.h"
#include "phj_mat.h"
#include "phj_partition.h"
#include "phj_hot.h"
#include "phj_table.h"
#include "phj_member.h"
#include "phj_lookup.h"

using namespace phj;

namespace {

constexpr double kNPDefaultRatio = 2.0;             // slots per build tuple
constexpr uint32_t kNPRegionBuckets = 1024;           // NoPartitioning region build: buckets per region (LDS 60 B each)
constexpr int kOnePassMax = 256;                      // hash % P: largest P partitioned in one pass

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
};

// Launch-shape knobs (results never depend on them). Defaults are the tuned
// values; ctx_create_device reads their PHJ_* overrides (every one is run by
// tests/test_gpu_schedules.py).
struct Tuning {
    int tile = 4096;      // tile kernels: tuples per tile (2048, 4096 or 8192)
    int block = 512;      // threads per workgroup of the tile kernels (256, 512 or 1024; tile_shape)
    int nt_load = 1;      // nontemporal tuple loads in the partition passes: 1 pass 1, 2 both
    bool fused = true;    // radix join: fused per-partition LDS build + probe when partitions are small
    int ptab = 1;         // partitioned bucket tables: 0 never, 1 very large partitions, 2 always
    bool subpart = true;  // phj_join: sub-partition large partitions for the fused join
    bool timers = true;   // per-kernel timer events (phase events are always recorded)
    bool p1_chunk = true; // 2-pass, unordered partitions: chunked pass 1 without a histogram pass
    int p1_slots = 0;     // chunked pass 1: workgroups per shard (0 = fill the chip once, -1 = one per tile)
    int p1_wpc2 = 2;      // ... keys-only: workgroups per CU x 2 (0 = fill the chip once)
    int p1_tps = static_cast<int>(kTilesPerShard);   // chunked pass 1: tiles per shard (sets the shard count)
    int p1_min_tiles = 32768;  // chunked pass 1: smallest relation (in 4096-tuple tiles, ~134M tuples)
    int p1_ko_tps = 1024;      // ... the keys-only form for the on-chip probe: tiles per shard (at every size)
    int p2probe = 1;      // radix join, 2 passes: the probe side's pass 2 on-chip (k_probe_ht)
    int p1_pipe = 1;      // keys-only pass 1: claims resolved a tile later over pre-allocated chunks (k_chunk_codes_pipe)
    int r_chunk = 1;      // LDS join on one device: R through the chunked code pass, read by tiles ("tile mode")
    int count_pin = 1;    // LDS join: the last workgroup writes the count to pinned host memory (0: a copy back)
    int r_order = 1;      // LDS join: R's pass 1 beside S's (0), after it (1: measured C2 1.69 vs 1.72 ms, S.p1 1.05 vs 1.19), before it (2)
    int p1_block = 1024;  // ... its workgroup: 1024 x 4 codes (16 waves per CU; measured 1.20 -> 1.07 ms at C2) or 512 x 8, the same tile
    int cluster = 1;      // radix join: LDS cluster tables (phj_cluster.h) when the build side's clusters fit
    int cl_cap = static_cast<int>(kClCapMax);   // ... LDS table slots (8192: two workgroups per CU, 16384: one)
    int cl_bits = 0;      // ... clusters = 2^cl_bits (0: the fewest >= 256 whose average fits the table)
};

// f(std::integral_constant<int, HK>) for the hash kind hk: a kernel template
// over the hash is named once per launch site, as <decltype(h)::value>.
template <class F>
auto with_hash(int hk, F f) {
    return hk == kMurmur3 ? f(std::integral_constant<int, kMurmur3>{}) : f(std::integral_constant<int, kXXH3>{});
}

// ... and f(std::true_type / std::false_type) for a kernel template over a bool.
template <class F>
auto with_bool(bool b, F f) {
    return b ? f(std::true_type{}) : f(std::false_type{});
}

int env_int(const char* name, int dflt) {
    const char* v = std::getenv(name);
    return (v && *v) ? std::atoi(v) : dflt;
}

struct Plan {
    int hk = 0;
    uint64_t seed = 0;
    uint32_t mode = 0;    // 0: q = h & (P-1), 1: q = h % P
    uint64_t P = 0;       // logical partitions
    uint32_t npass = 1;
    uint32_t nb1 = 1, nb2 = 1;
    uint32_t bits1 = 0, bits2 = 0;
    uint32_t shift1 = 0, dmask1 = 0, dmask2 = 0;
    uint32_t Ppad = 1;    // nb1 * nb2 = final bounds length - 1
    uint32_t sub_bits = 0, sub_shift = 0;   // phj_join: sub-partitions per partition (refine_plan)
    bool stable = false;  // PHJ_PART_STABLE: the reference's order inside each partition (not compared by ==)
    bool chained = false; // PHJ_TABLE_CHAINED: bucket-chained (CSR) tables in HBM (not compared by ==: tables only)
    bool cluster = false; // phj_join: pass 1 = the LDS join's clusters (cluster_plan), the count path of phj_cluster.h
    bool operator==(const Plan& o) const {
        return hk == o.hk && seed == o.seed && mode == o.mode && P == o.P && npass == o.npass &&
               nb1 == o.nb1 && nb2 == o.nb2 && sub_bits == o.sub_bits && sub_shift == o.sub_shift;
    }
};

struct TimerRec {
    std::string name;
    uint64_t bytes;
    hipEvent_t a, b;
    int split = 0;   // 1 / 2: the build / probe share of a fused join launch (ctx->split clocks)
};

struct SideState {
    const phj_tuple* rel = nullptr;
    uint64_t n = 0;
    DevBuf owned;
    // bound as columns (phj_relation_bind_columns ...): the key column and the
    // payload column (null: keys alone), borrowed or in ck / cp. rel is then
    // null until a call without a column form packs the tuple copy `pack`
    // (need_tuples), kept until the side is rebound
    bool columns = false, cols_owned = false, packed = false;
    const int64_t* ckeys = nullptr;
    const int64_t* cpays = nullptr;
    DevBuf ck, cp, pack;
    DevBuf kA, pA, kB, pB;
    DevBuf hist1, hist2, bounds1, tbase2, tseg2, bounds, partials;
    DevBuf dig;           // pass-2 digit column written by pass 1
    DevBuf ccur, ctab, tstart;   // chunked pass 1: digit cursors + pool counter, chunk table, pass-2 tile starts
    DevBuf csink;                // ... code form: sink words of the stores past the tile (never read)
    bool ctab_dirty = true;      // chunked pass 1: the chunk table may hold entries (clear before the next pass)
    bool hcoded = false;         // the last pass 1 wrote hash codes (keys only, k_chunk_codes)
    bool chunk_check = false;    // a chunked pass ran whose error word (chunk_err_word) nobody has read yet
    phj_partitioned view{};
    PassArgs p2{};               // p1_only: the pass-2 tile mapping over the pass-1 output
    uint32_t nt2 = 0;            // ... and its tile bound
    bool partitioned = false;
    Plan plan;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
};

uint32_t ceil_log2(uint64_t x) {
    uint32_t b = 0;
    while ((1ull << b) < x) b++;
    return b;
}

uint32_t next_pow2_u32(uint32_t x) {
    uint32_t p = 1;
    while (p < x) p <<= 1;
    return p;
}

struct Group;   // phj_group.h: the members of a multi-device context

}  // namespace

struct phj_ctx {
    Group* group = nullptr;        // multi-device context (phj_group.h); null for one device
    int device = 0;
    hipStream_t stream = nullptr;  // the ctx stream (own or borrowed)
    hipStream_t aux = nullptr;     // ctx-owned: R-side partitioning runs here beside S
    hipStream_t ks = nullptr;      // stream the current launches go to (stream or aux)
    DevBuf* scan_scratch = nullptr; // scan partials of the side being partitioned
    int num_cus = 256;
    bool own_stream = false;
    SideState side[2];
    DevBuf scan_partials, prep, tkeys, tpays, toffs, gcursor, items, count, biglist;
    DevBuf ht_tab, ht_desc;   // on-chip join: code tables, descriptors (build_ht)
    DevBuf r_codes, r_bounds;         // ... the build side's codes in partition order and bounds (single device)
    DevBuf np_tab, np_pays;
    DevBuf np_ovf, np_ovfb, np_ovfn;   // region build: overflow tuples, their start buckets, count
    DevBuf np_uni;                     // code-table NoPartitioning: {uniform?, cap} (k_np_ct_plan)
    DevBuf member_marks;               // phj_join_member: one byte per slot of ht_tab (cleared before each join that marks)
    DevBuf fitems, split, cl_prof;
    DevBuf mat_mark, mat_cnt, mat_rows;   // materialised join: per-probe match, block offsets, rows
    DevBuf row_hit, row_only, row_cnt;    // phj_join_rows: build hit flags, probe-only bitmap, build block offsets
    DevBuf agg_acc, agg_cnt, agg_rows, agg_res;   // phj_join_aggregate: accumulator planes, block offsets, group rows, {5 totals, rows}
    uint64_t agg_n = 0;   // group rows of the last phj_join_aggregate
    uint64_t mat_n = 0;   // fused join: item slots; wave clocks {build, probe} since the last timer reset
    // phj_join_indices: its two index columns lie in mat_rows, build_rows in
    // int64 words [0, idx_n), probe_rows in [idx_n, 2 idx_n) (16 B per row
    // where a materialised join holds 24: one result at a time, so whichever
    // join ran last zeroes the other's count)
    uint64_t idx_n = 0;
    DevBuf gather_bad;    // phj_gather_column: its count of indices out of range
    std::vector<hipEvent_t> evpool;
    size_t evnext = 0;
    std::vector<TimerRec> timers;
    std::string err;
    Tuning tune;
    bool last_fused = false;   // the last build_and_probe ran the fused kernel
    bool dry = false;          // phj_prepare: size and allocate the workspace, launch nothing
    hipEvent_t last_ev = nullptr;      // the last event recorded (mark) ...
    hipStream_t last_ev_stream = nullptr;  // ... on this stream ...
    uint32_t since_ev = 0;             // ... and the kernels launched since
    unsigned long long* count_host = nullptr;   // pinned: the count read back
    // fine-grained pinned {count, failed} written by the LDS join's last
    // workgroup (k_cluster_probe_big), its device address, and the launch's
    // finished-workgroup counter; count_pinned: this join's count is there
    unsigned long long* count_pin = nullptr;
    unsigned long long* count_pin_dev = nullptr;
    DevBuf cl_done;
    bool count_pin_failed = false, count_pinned = false;
    unsigned long long* split_words = nullptr;  // the LDS probe's {build, probe} clocks (count buffer words 2-3), this join
    bool defer_timers = false;  // the running join has PHJ_DEFER_TIMERS: its timers stay for phj_timers_report
    bool lean_timers = false;   // PHJ_LEAN_TIMERS: the build side's timers are not recorded
    bool timer_skipped = false; // the open timer was not recorded (timer_end records nothing)
    // the next chunked pass-1 bookkeeping kernel also clears this chunk state
    // (the LDS join: R's, cleared by S's k_pass1_finish_sizes on the same
    // stream), and the pass whose state p1_cleared names skips its memset
    void* p1_clear = nullptr;
    size_t p1_clear_bytes = 0;
    void* p1_cleared = nullptr;
    // the probe side's chunk state left all zero by the last join's final
    // workgroup (k_cluster_probe_big, s_clear) and its size; pending: asked
    // of the running join, confirmed when its count shows no failure
    void* s_zeroed = nullptr;
    size_t s_zeroed_bytes = 0;
    void* s_zero_pending = nullptr;
    size_t s_zero_pending_bytes = 0;
    int poison = -1;   // phj_debug_poison_alloc: every new workspace buffer is filled with this byte
    // hot-key pre-aggregation (phj_hot.h): the state; phj_debug_preagg's mode
    // (0 auto, 1 off, 2 forced); hot_on: the running join's probe-side code
    // pass takes its HOT form; hot_ran / hot_n / hot_min_mass: the last join's, for its statistics
    // hot_clean / hot_clean_nb: the buffer and cluster count for which the
    // counters and control words are known to be zero (k_hot_select's
    // clearing); else the next prologue starts with k_hot_clear
    DevBuf hot;
    void* hot_clean = nullptr;
    uint32_t hot_clean_nb = 0;
    int hot_mode = 0;
    bool hot_on = false, hot_ran = false;
    uint64_t hot_n = 0;
    uint32_t hot_min_mass = 0;
    // R's chain beside the hot-key prologue: the aux stream
    // waits for hot_fork (the main stream at the join's start), the main
    // stream for hot_join (the end of R's chain); p1_free_cus: CUs per shard
    // the chunked pass 1 launched next leaves free
    hipEvent_t hot_fork = nullptr, hot_join = nullptr;
    uint32_t p1_free_cus = 0;
    bool p1_cols = false;   // the chunked pass 1 launched next reads a key column (partition_state, cols_native)
    std::vector<phj_index*> indexes;   // phj_index_build: the live indexes (each owns its table; destroy frees survivors)
};

// A retained key index (phj_lookup.h): its table is memory of its own, not
// workspace, so no later join, rebind or grow of the context touches it.
struct phj_index {
    phj_ctx* owner = nullptr;
    IxBucket* tab = nullptr;
    size_t bytes = 0;
    NPHome g{};
    int hk = 0;
    uint64_t seed = 0;
    uint64_t rows = 0, distinct = 0;
    uint32_t max_wgs = 1;   // workgroups that fill the chip once at the lookup's occupancy
    // PHJ_INDEX_ORDINALS (phj_ordinal.h): the slots hold ordinals; first_rows[ordinal] = the key's first row
    uint32_t flags = 0;
    int64_t* first_rows = nullptr;   // `distinct` entries, the index's own memory (counted in bytes)
    uint32_t acc_wgs = 1;            // max_wgs of k_ix_accumulate
};

namespace {

int set_err(phj_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg;
    return code;
}

#define PHJ_HIP(ctx, expr)                                                                   \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess)                                                                \
            return set_err(ctx, PHJ_ERR_HIP,                                                 \
                           std::string(#expr) + ": " + hipGetErrorString(e_));               \
    } while (0)

#define PHJ_LAUNCHED(ctx, what)                                                              \
    do {                                                                                     \
        (ctx)->since_ev++;                                                                   \
        hipError_t e_ = hipGetLastError();                                                   \
        if (e_ != hipSuccess)                                                                \
            return set_err(ctx, PHJ_ERR_HIP, std::string("launch ") + what + ": " +         \
                                                 hipGetErrorString(e_));                     \
    } while (0)

#define PHJ_TRY(expr)           \
    do {                        \
        int rc_ = (expr);       \
        if (rc_ != PHJ_OK) return rc_; \
    } while (0)

int ensure(phj_ctx* c, DevBuf& b, size_t bytes) {
    if (bytes == 0) bytes = 16;
    if (b.bytes >= bytes) return PHJ_OK;
    if (b.p) {
        PHJ_HIP(c, hipStreamSynchronize(c->stream));
        PHJ_HIP(c, hipStreamSynchronize(c->aux));
        PHJ_HIP(c, hipFree(b.p));
        b.p = nullptr;
        b.bytes = 0;
    }
    const size_t rounded = (bytes + 4095) & ~size_t(4095);
    hipError_t e = hipMalloc(&b.p, rounded);
    if (e != hipSuccess) {
        b.p = nullptr;
        return set_err(c, PHJ_ERR_NOMEM, "hipMalloc(" + std::to_string(rounded) + "): " + hipGetErrorString(e));
    }
    b.bytes = rounded;
    if (c->poison >= 0) {   // (test hook) no buffer may be read before it is written
        PHJ_HIP(c, hipMemsetAsync(b.p, c->poison, rounded, c->stream));
        PHJ_HIP(c, hipStreamSynchronize(c->stream));
    }
    return PHJ_OK;
}

void free_buf(DevBuf& b) {
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.bytes = 0;
}

hipEvent_t new_event() {
    hipEvent_t e = nullptr;
    // timing / same-device ordering only: no system-scope fence (a default
    // event's system-scope writeback costs ~10 us per record); the first
    // flag set the runtime accepts is used
    const unsigned tries[3] = {hipEventDisableSystemFence, hipEventReleaseToDevice, hipEventDefault};
    for (unsigned f : tries) {
        if (hipEventCreateWithFlags(&e, f) == hipSuccess) break;
        (void)hipGetLastError();
        e = nullptr;
    }
    return e;
}

hipEvent_t next_event(phj_ctx* c) {
    if (c->evnext == c->evpool.size()) {
        hipEvent_t e = new_event();
        if (!e) return nullptr;
        c->evpool.push_back(e);
    }
    return c->evpool[c->evnext++];
}

// phj_prepare: events for this many timer marks created up front (deferred
// timers keep every join's marks until phj_timers_report, ~4 per join under
// PHJ_LEAN_TIMERS: 64 joins' worth), so no hipEventCreate runs inside a timed loop
constexpr size_t kPrepEvents = 256;
int reserve_events(phj_ctx* c, size_t n) {
    while (c->evpool.size() < n) {
        hipEvent_t e = new_event();
        if (!e) return set_err(c, PHJ_ERR_HIP, "hipEventCreate failed");
        c->evpool.push_back(e);
    }
    if (c->timers.capacity() < n) c->timers.reserve(n);
    return PHJ_OK;
}

int mark(phj_ctx* c, hipEvent_t* out) {
    *out = next_event(c);
    if (!*out) return set_err(c, PHJ_ERR_HIP, "hipEventCreate failed");
    PHJ_HIP(c, hipEventRecord(*out, c->ks));
    c->last_ev = *out;
    c->last_ev_stream = c->ks;
    c->since_ev = 0;
    return PHJ_OK;
}

// mark, or the last event when it was recorded on this stream with nothing
// launched after it (the same point of the stream: one marker packet fewer)
int mark_shared(phj_ctx* c, hipEvent_t* out) {
    if (c->last_ev && c->last_ev_stream == c->ks && c->since_ev == 0) {
        *out = c->last_ev;
        return PHJ_OK;
    }
    return mark(c, out);
}

int timer_begin(phj_ctx* c, const char* name, uint64_t bytes) {
    if (!c->tune.timers) return PHJ_OK;
    c->timer_skipped = c->lean_timers && (std::strncmp(name, "R.", 2) == 0 || std::strcmp(name, "build.big") == 0);
    if (c->timer_skipped) return PHJ_OK;   // PHJ_LEAN_TIMERS
    TimerRec t{name, bytes, nullptr, nullptr};
    // back-to-back timers on one stream share the boundary event (the previous
    // timer's end is this one's start when nothing was launched in between)
    if (c->last_ev && c->last_ev_stream == c->ks && c->since_ev == 0) t.a = c->last_ev;
    else PHJ_TRY(mark(c, &t.a));
    c->timers.push_back(t);
    return PHJ_OK;
}

// Launch kfn on the current launch stream.
int launch_kernel(phj_ctx* c, const void* kfn, dim3 grid, dim3 block, void** args, size_t lds, const char* what) {
    PHJ_HIP(c, hipLaunchKernel(kfn, grid, block, args, lds, c->ks));
    PHJ_LAUNCHED(c, what);
    return PHJ_OK;
}

int timer_end(phj_ctx* c) {
    if (c->timer_skipped) {
        c->timer_skipped = false;
        return PHJ_OK;
    }
    return c->tune.timers ? mark(c, &c->timers.back().b) : PHJ_OK;
}

// One launch reported as two timers (build, probe) split by the kernel's own clocks.
int timer_begin_split(phj_ctx* c, uint64_t build_bytes, uint64_t probe_bytes) {
    if (!c->tune.timers) return PHJ_OK;
    PHJ_TRY(timer_begin(c, "build", build_bytes));
    c->timers.back().split = 1;
    c->timers.push_back(TimerRec{"probe", probe_bytes, c->timers.back().a, nullptr, 2});
    return PHJ_OK;
}

int timer_end_split(phj_ctx* c) {
    if (!c->tune.timers) return PHJ_OK;
    PHJ_TRY(mark(c, &c->timers.back().b));
    c->timers[c->timers.size() - 2].b = c->timers.back().b;
    return PHJ_OK;
}

constexpr size_t kMaxTimerRecs = 1u << 14;

void reset_timers(phj_ctx* c) {
    c->timers.clear();
    c->evnext = 0;
    c->last_ev = nullptr;
    c->split_words = nullptr;
    if (c->split.p) (void)hipMemsetAsync(c->split.p, 0, 16, c->ks);
}

// What every entry point that launches work does once its arguments are
// checked: a stale error left by code outside this library is dropped, the
// device selected, and the per-call state set: the timer flags of this call
// (PHJ_DEFER_TIMERS / PHJ_LEAN_TIMERS of phj_join's params, else none), no open
// timer, no pinned count of an earlier join, launches on the ctx stream.
// Timers: reset, unless this call defers them or (accumulate: phj_partition
// and the calls over its output, which report them together) adds to them;
// a caller that never reports loses the oldest records.
// Every such entry point clears all of it: before they shared this prologue,
// phj_join_materialize, phj_probe_pass1, phj_partition, phj_join_partitioned(_async)
// and phj_relation_count_in_range left count_pinned and timer_skipped (and the
// last three the timer flags) as the call before them had, so that after an LDS
// join that failed between its probe and get_count they read that join's pinned count.
int begin_call(phj_ctx* c, uint32_t timer_flags = 0, bool accumulate = false) {
    (void)hipGetLastError();
    PHJ_HIP(c, hipSetDevice(c->device));
    c->defer_timers = (timer_flags & PHJ_DEFER_TIMERS) != 0;
    c->lean_timers = (timer_flags & PHJ_LEAN_TIMERS) != 0;
    c->timer_skipped = false;
    c->count_pinned = false;
    c->ks = c->stream;
    if (!(accumulate || c->defer_timers) || c->timers.size() > kMaxTimerRecs) reset_timers(c);
    return PHJ_OK;
}

// Build share of the fused join launches since the last reset (wave clocks).
double fused_build_fraction(phj_ctx* c) {
    unsigned long long cyc[2] = {0, 0};
    const void* src = c->split_words ? static_cast<const void*>(c->split_words) : c->split.p;
    if (!src || hipMemcpyAsync(cyc, src, 16, hipMemcpyDeviceToHost, c->ks) != hipSuccess ||
        hipStreamSynchronize(c->ks) != hipSuccess)
        return 0.5;
    const double t = static_cast<double>(cyc[0]) + static_cast<double>(cyc[1]);
    return t > 0 ? static_cast<double>(cyc[0]) / t : 0.5;
}

// Timers aggregated by name (sums over every record since the last reset:
// one join, or many when a caller reports once after several joins).
int fill_timers(phj_ctx* c, phj_join_result* r) {
    r->num_timers = 0;
    if (c->defer_timers) return PHJ_OK;   // PHJ_DEFER_TIMERS: read later by phj_timers_report
    double fb = -1.0;
    for (const TimerRec& t : c->timers) {
        float ms = 0;
        PHJ_HIP(c, hipEventElapsedTime(&ms, t.a, t.b));
        if (t.split) {
            if (fb < 0) fb = fused_build_fraction(c);
            ms = static_cast<float>(ms * (t.split == 1 ? fb : 1.0 - fb));
        }
        uint32_t i = 0;
        while (i < r->num_timers && std::strncmp(r->timer_name[i], t.name.c_str(), PHJ_TIMER_NAME - 1) != 0) i++;
        if (i == r->num_timers) {
            if (r->num_timers >= PHJ_MAX_TIMERS) continue;
            r->num_timers++;
            r->timer_ms[i] = 0;
            r->timer_bytes[i] = 0;
            std::snprintf(r->timer_name[i], PHJ_TIMER_NAME, "%s", t.name.c_str());
        }
        r->timer_ms[i] += ms;
        r->timer_bytes[i] += t.bytes;
    }
    return PHJ_OK;
}

double elapsed(phj_ctx* c, hipEvent_t a, hipEvent_t b) {
    if (c->defer_timers) return 0.0;   // PHJ_DEFER_TIMERS: no event queries in the join
    float ms = 0;
    if (hipEventElapsedTime(&ms, a, b) != hipSuccess) return -1.0;
    return ms;
}

int make_plan(phj_ctx* c, const phj_join_params* p, Plan& pl) {
    if (!p) return set_err(c, PHJ_ERR_INVALID, "null params");
    if (p->hash != PHJ_HASH_XXH3 && p->hash != PHJ_HASH_MURMUR3)
        return set_err(c, PHJ_ERR_INVALID, "unknown hash function");
    pl = Plan{};
    pl.stable = (p->flags & PHJ_PART_STABLE) != 0;
    pl.chained = (p->flags & PHJ_TABLE_CHAINED) != 0;
    pl.hk = p->hash;
    pl.seed = p->hash_seed;
    if (p->num_partitions > 0) {
        pl.mode = 1;
        pl.P = p->num_partitions;
        // one pass while the scatter's runs stay long (a 4096-tuple tile over
        // <= 256 digits); beyond, two passes with balanced digits: pass 1 on
        // q >> b2, pass 2 on q & (2^b2 - 1), 2^b2 ~ sqrt(P)
        if (pl.P <= static_cast<uint64_t>(kOnePassMax)) {
            pl.npass = 1;
            pl.nb1 = static_cast<uint32_t>(pl.P);
            pl.bits1 = ceil_log2(pl.P);
            pl.shift1 = 0;
            pl.dmask1 = 0xffffffffu;
        } else {
            if (pl.P > (1ull << (2 * kMaxDigitBits)))
                return set_err(c, PHJ_ERR_RANGE, "num_partitions above 2^22");
            const uint32_t b2 = std::min<uint32_t>(kMaxDigitBits, (ceil_log2(pl.P) + 1) / 2);
            pl.npass = 2;
            pl.nb2 = 1u << b2;
            pl.bits2 = b2;
            pl.nb1 = static_cast<uint32_t>((pl.P + pl.nb2 - 1) / pl.nb2);
            pl.bits1 = ceil_log2(pl.nb1);
            pl.shift1 = b2;
            pl.dmask1 = 0xffffffffu;
            pl.dmask2 = pl.nb2 - 1;
        }
    } else {
        const uint32_t b0 = p->radix_bits[0], b1 = p->radix_bits[1];
        if (b0 < 1 || b0 > static_cast<uint32_t>(kMaxDigitBits) || b1 > static_cast<uint32_t>(kMaxDigitBits))
            return set_err(c, PHJ_ERR_INVALID, "radix_bits must be in [1,11] x [0,11]");
        pl.mode = 0;
        pl.P = 1ull << (b0 + b1);
        pl.nb1 = 1u << b0;
        pl.bits1 = b0;
        pl.dmask1 = pl.nb1 - 1;
        pl.shift1 = b1;
        if (b1 == 0) {
            pl.npass = 1;
        } else {
            pl.npass = 2;
            pl.nb2 = 1u << b1;
            pl.bits2 = b1;
            pl.dmask2 = pl.nb2 - 1;
        }
    }
    pl.Ppad = pl.nb1 * pl.nb2;
    return PHJ_OK;
}

// phj_join only: when the requested partitions are too large for the fused LDS
// join (the reference's -p 32 .. 8192 at 10M build tuples), split every
// partition into 2^s sub-partitions of ~<= 170 build tuples (DigitFn sub_bits)
// and partition on the refined q in two balanced passes. The count is the
// same (a partition's hash table is simply organised by further hash bits);
// phj_partition keeps the exact layout of the requested partitions.
void refine_plan(const phj_ctx* c, Plan& pl, uint64_t nR) {
    if (!c->tune.subpart || !c->tune.fused || pl.P == 0) return;
    const double expect = static_cast<double>(nR) / static_cast<double>(pl.P);
    if (expect * 3 <= static_cast<double>(kFusedTcap) * 2) return;
    const uint32_t logP = ceil_log2(pl.P);
    uint32_t s = 0;
    while (expect / static_cast<double>(1ull << s) > 170.0 && logP + s < 2u * kMaxDigitBits) s++;
    if (s == 0) return;
    pl.sub_bits = s;
    // radix: the hash bits just above the partition bits; hash % P: bits 40+
    // (the LDS table buckets use bits 32..39)
    pl.sub_shift = pl.mode == 0 ? logP : 40;
    const uint64_t range = (pl.mode == 0 ? (1ull << logP) : pl.P) << s;
    const uint32_t b2 = std::min<uint32_t>(kMaxDigitBits, (ceil_log2(range) + 1) / 2);
    pl.npass = 2;
    pl.nb2 = 1u << b2;
    pl.bits2 = b2;
    pl.dmask2 = pl.nb2 - 1;
    pl.nb1 = static_cast<uint32_t>((range + pl.nb2 - 1) / pl.nb2);
    pl.bits1 = ceil_log2(pl.nb1);
    pl.shift1 = b2;
    pl.dmask1 = 0xffffffffu;
    pl.Ppad = pl.nb1 * pl.nb2;
}

// The LDS join's plan (phj_cluster.h) from the requested one (make_plan):
// pass 1 partitions into K = 2^k clusters, the top k bits of the partition
// number q (refined by sub-partition bits when q has fewer than k bits: hash
// bits just above the radix bits, or bits 40+ under h % P, as refine_plan),
// so every cluster is a union of whole requested partitions. K is the smallest
// power of two >= 256 (chains enough for S's pass-1 cursors) whose average
// cluster fills at most 0.8 of the LDS limit (the binomial spread of the
// cluster sizes, ~3 % at 10M / 1024); larger build sides than 2048 clusters
// hold take the code-table path. Returns false when the plan does not apply.
bool cluster_plan_k(const Plan& base, uint32_t k, Plan& pl) {
    pl = base;
    pl.cluster = true;
    pl.sub_bits = 0;
    pl.sub_shift = 0;
    uint32_t bits;   // bits of the (refined) partition number
    if (base.mode == 0) {
        const uint32_t logP = ceil_log2(base.P);
        if (logP < k) {
            pl.sub_bits = k - logP;
            pl.sub_shift = logP;
        }
        bits = std::max(logP, k);
    } else {
        uint32_t s = 0;
        while ((base.P << s) < (1ull << k)) s++;
        if (s) {
            pl.sub_bits = s;
            pl.sub_shift = 40;
        }
        bits = ceil_log2(base.P << s);
    }
    const uint64_t range = (base.mode == 0 ? (1ull << ceil_log2(base.P)) : base.P) << pl.sub_bits;
    const uint32_t shift = bits - k;
    pl.npass = 2;
    pl.shift1 = shift;
    pl.dmask1 = 0xffffffffu;
    pl.nb1 = static_cast<uint32_t>((range + (1ull << shift) - 1) >> shift);
    pl.bits1 = ceil_log2(pl.nb1);
    pl.nb2 = 1u << shift;
    pl.bits2 = shift;
    pl.dmask2 = pl.nb2 - 1;
    pl.Ppad = pl.nb1 * pl.nb2;
    return pl.nb1 >= 2 && pl.nb1 <= static_cast<uint32_t>(kMaxBins);
}

bool cluster_plan(const phj_ctx* c, const Plan& base, uint64_t nR, Plan& pl) {
    if (!c->tune.cluster || base.chained || nR == 0 || base.P == 0) return false;
    const double fit = 0.8 * cl_lim(static_cast<uint32_t>(c->tune.cl_cap));
    // h % P: the clusters are 2^shift consecutive refined partitions each, so
    // there may be fewer than 2^k of them; every k is tried until they fit
    const uint32_t k0 = c->tune.cl_bits > 0 ? static_cast<uint32_t>(c->tune.cl_bits) : 8;
    const uint32_t k1 = c->tune.cl_bits > 0 ? k0 : static_cast<uint32_t>(kMaxDigitBits);
    for (uint32_t k = k0; k <= k1; k++)
        if (cluster_plan_k(base, k, pl) && static_cast<double>(nR) / static_cast<double>(pl.nb1) <= fit) return true;
    return false;
}

DigitFn digit_fn(const Plan& pl, int pass) {
    DigitFn f{};
    f.seed = pl.seed;
    f.P = pl.P;
    f.mode = pl.mode;
    f.magic = pl.mode == 1 ? (~0ull) / pl.P : 0;
    f.sub_bits = pl.sub_bits;
    f.sub_shift = pl.sub_shift;
    if (pass == 1) {
        f.shift = pl.shift1;
        f.dmask = pl.dmask1;
    } else {
        f.shift = 0;
        f.dmask = pl.dmask2;
    }
    return f;
}


// E_0 of the plan's code tables (phj_table.h ht_empty): the lowest power of
// two whose final partition is not 0. Code 0 is in partition 0 under every
// partition function, so E_p = 0 serves every other partition. 1 for radix bits
// and h % P with P >= 2; 2^40 for h % 1 split into sub-partitions at bit 40
// (code 1 is in partition 0 there); 0 when the plan has one final partition
// (no code lies elsewhere: use_p2probe then declines the code tables).
uint64_t plan_empty0(const Plan& pl) {
    const DigitFn f = digit_fn(pl, 1);
    for (int b = 0; b < 64; b++)
        if (q_from_hash(1ull << b, f) != 0) return 1ull << b;
    return 0;
}

// E of cluster 0 (phj_cluster.h): the lowest power of two outside cluster 0
// (pass-1 digit 0); 0 when every code is in cluster 0.
uint64_t cluster_empty0(const Plan& pl) {
    const DigitFn f = digit_fn(pl, 1);
    for (int b = 0; b < 64; b++)
        if (((q_from_hash(1ull << b, f) >> f.shift) & f.dmask) != 0) return 1ull << b;
    return 0;
}

int scan_u32(phj_ctx* c, uint32_t* data, uint32_t len, uint32_t narrays, uint32_t stride,
             DevBuf* scratch = nullptr) {
    if (len == 0) return PHJ_OK;
    ScanArgs s{};
    s.data = data;
    s.len = len;
    s.stride = stride;
    s.nblk = (len + kScanBlockElems - 1) / kScanBlockElems;
    DevBuf& part = scratch ? *scratch : c->scan_partials;
    PHJ_TRY(ensure(c, part, static_cast<size_t>(s.nblk) * narrays * 4));
    if (c->dry) return PHJ_OK;
    s.partials = static_cast<uint32_t*>(part.p);
    hipLaunchKernelGGL(k_scan_reduce, dim3(s.nblk, narrays), dim3(kBlock), 0, c->ks, s);
    PHJ_LAUNCHED(c, "k_scan_reduce");
    hipLaunchKernelGGL(k_scan_apply, dim3(s.nblk, narrays), dim3(kBlock), 0, c->ks, s);
    PHJ_LAUNCHED(c, "k_scan_apply");
    return PHJ_OK;
}


// The pipelined code pass in 1024 x 4 workgroups: KPF tiles of keys in
// flight (S: 2, measured 1.08 -> 1.05 ms at C2; R: 1); a measurement build
// (-DPHJ_P1_PROF=1, scripts/ab_lib.sh) runs S's pass in the phase-clock form.
// cols: the relation is a key column (k_chunk_codes_pipe COLS 1, one digit
// per thread only: cols_native).
template <int HK, int DPT>
const void* pipe1024(int kpf, bool hot = false, bool cols = false) {
    if constexpr (DPT == 1 && PHJ_PREAGG != 0) {   // the HOT form (phj_hot.h): S's pass counts the hot codes' weights
        if (hot && kpf != 1)
            return cols ? reinterpret_cast<const void*>(&k_chunk_codes_pipe<1024, 4, HK, 1, 0, PHJ_P1_PROF != 0, 2, 1, 1>)
                        : reinterpret_cast<const void*>(&k_chunk_codes_pipe<1024, 4, HK, 1, 0, PHJ_P1_PROF != 0, 2, 1, 0>);
    }
    if constexpr (DPT == 1) {
        if (cols) {
            if (kpf == 1) return reinterpret_cast<const void*>(&k_chunk_codes_pipe<1024, 4, HK, 1, 0, false, 1, 0, 1>);
            return reinterpret_cast<const void*>(&k_chunk_codes_pipe<1024, 4, HK, 1, 0, false, 2, 0, 1>);
        }
    }
    if (kpf == 1) return reinterpret_cast<const void*>(&k_chunk_codes_pipe<1024, 4, HK, DPT, 0, false, 1>);
    return reinterpret_cast<const void*>(&k_chunk_codes_pipe<1024, 4, HK, DPT, 0, PHJ_P1_PROF != 0, 2>);
}

// Workgroups per CU of kernel kfn at `block` threads and `lds` bytes of dynamic
// LDS, as the runtime reports it (0 if it cannot), cached per host thread: the
// query reads the kernel's attributes through the runtime, host time before
// every launch of a join otherwise.
int occupancy(const void* kfn, int block, size_t lds) {
    struct Key {
        const void* f;
        int b;
        size_t l;
        bool operator==(const Key& o) const { return f == o.f && b == o.b && l == o.l; }
    };
    struct Hash {
        size_t operator()(const Key& k) const {
            return std::hash<const void*>()(k.f) ^ (static_cast<size_t>(k.b) << 20) ^ (k.l * 0x9E3779B97F4A7C15ull);
        }
    };
    thread_local std::unordered_map<Key, int, Hash> cache;
    const Key k{kfn, block, lds};
    auto it = cache.find(k);
    if (it != cache.end()) return it->second;
    int occ = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kfn, block, lds) != hipSuccess) {
        (void)hipGetLastError();
        occ = 0;
    }
    cache.emplace(k, occ);
    return occ;
}

// ... or `fallback` where the runtime cannot tell.
int occupancy_or(const void* kfn, int block, size_t lds, int fallback) {
    const int occ = occupancy(kfn, block, lds);
    return occ < 1 ? fallback : occ;
}

// A grid of `want` workgroups, at most per_cu on every CU, at least one.
uint32_t chip_grid(const phj_ctx* c, uint64_t want, int per_cu) {
    return static_cast<uint32_t>(std::max<uint64_t>(1, std::min<uint64_t>(want, static_cast<uint64_t>(per_cu) * c->num_cus)));
}

// ROWS (pass 1 of the row-number joins, phj_index.h): 0 = the payloads are
// loaded; 1 / 2 = the input is a key column / 16-B tuples whose payloads are
// ignored, and the payload written is the tuple's row number. Only the passes
// that move whole tuples have these forms (IN_AOS, never keys_only).
template <int BLOCK, int ITEMS, bool IN_AOS, bool OUT_AOS, int ROWS = 0>
int launch_pass_t(phj_ctx* c, int hk, const PassArgs& a, uint32_t grid, const std::string& prefix,
                  uint64_t n, uint32_t hist_len) {
    static_assert(ROWS == 0 || IN_AOS, "row numbers are synthesised by pass 1");
    if (ROWS != 0 && a.keys_only) return set_err(c, PHJ_ERR_INVALID, "row-number pass 1: no keys-only form");
    constexpr uint64_t kcol = ROWS == 1 ? 8 : 0;   // bytes per tuple a key column saves the reads
    constexpr int T = BLOCK * ITEMS;
    constexpr int NW = BLOCK / 64;
    const size_t hist_lds = static_cast<size_t>(NW) * a.nbins * 4;
    const size_t sc_lds = scatter_lds_bytes(T, a.nbins, NW, a.chunk_cursor != nullptr);
    const std::string hname = prefix + ".hist", cname = prefix + ".scan", sname = prefix + ".scatter";
    if (a.chunk_cursor) {
        // chunked pass 1: no histogram / scan; the digit cursors and the pool
        // counter start at zero
        const bool zeroed = a.chunk_cursor == c->s_zeroed && chunk_state_bytes(a.nbins) <= c->s_zeroed_bytes;
        if (a.chunk_cursor == c->s_zeroed) c->s_zeroed = nullptr;   // (this pass writes it)
        if (a.chunk_cursor == c->p1_cleared) c->p1_cleared = nullptr;   // cleared by the kernel before it
        else if (!zeroed) PHJ_HIP(c, hipMemsetAsync(a.chunk_cursor, 0, chunk_state_bytes(a.nbins), c->ks));
        c->since_ev++;
        // (a key column, c->p1_cols: 8 B read per tuple, not the 16-B tuple)
        const uint64_t sbytes = n * (a.keys_only ? 24 : 32) - (c->p1_cols ? n * 8 : 0) - n * kcol + (a.out_dig ? n * (a.dig_wide ? 2 : 1) : 0);
        PHJ_TRY(timer_begin(c, sname.c_str(), sbytes));
        if constexpr (IN_AOS && OUT_AOS && ITEMS <= 8) {
            // persistent: as many workgroups per shard as fit the chip at once
            // (two per CU at 81 KB of LDS), never more than the shard's tiles
            const uint32_t ntiles = static_cast<uint32_t>((n + T - 1) / T);
            const uint32_t per = (ntiles + a.nshards - 1) / a.nshards;
            const bool pipe = a.keys_only && c->tune.p1_pipe && BLOCK == 512 && ITEMS == 8;
            const bool is_r = prefix.rfind("R.", 0) == 0;
            const bool hot = a.hot_code != nullptr;   // S's pass only (the host offers it only where the 1024 x 4, one-digit-per-thread form runs)
            const size_t lds = pipe ? chunk_pipe_lds_bytes(T, a.nbins) + chunk_pipe_hot_lds_bytes(a.nbins, hot ? 1 : 0)
                               : a.keys_only ? chunk_codes_lds_bytes(T, a.nbins) : sc_lds;
            const void* kfn = nullptr;
            int kblock = BLOCK;
            bool cols_form = false;   // the kernel chosen reads a key column
            // keys only, written as hash codes (the on-chip probe): k_chunk_codes;
            // whole tuples: VAR 3, LDS-atomic ranking, 16-B LDS entries (phj_partition.h)
            // (more digits than threads: the cluster plans, 512 x 4096 only)
            if (a.keys_only && pipe) {
                if constexpr (BLOCK == 512 && ITEMS == 8) {
                    const int dpt = a.nbins > 2 * BLOCK ? 4 : a.nbins > BLOCK ? 2 : 1;
                    if (c->tune.p1_block == 1024) {   // 16 waves per CU, 4 codes per thread
                        kblock = 1024;
                        // R's pass (LDS join, tile mode: ~10 tiles per workgroup at C2)
                        // keeps one tile in flight, which also gives it a kernel name of
                        // its own in rocprof summaries (S's is the roofline kernel)
                        const int kpf = is_r ? 1 : 2;
                        if (hot && dpt == 4) return set_err(c, PHJ_ERR_STATE, "hot-key pre-aggregation: more digits than threads");
                        if (c->p1_cols && dpt == 4) return set_err(c, PHJ_ERR_STATE, "key column: more digits than threads");
                        const bool cols = c->p1_cols;
                        cols_form = cols;
                        kfn = with_hash(hk, [&](auto h) {
                            constexpr int HK = decltype(h)::value;
                            return dpt == 4 ? pipe1024<HK, 2>(kpf) : pipe1024<HK, 1>(kpf, hot, cols);
                        });
                    } else if (hot) {
                        return set_err(c, PHJ_ERR_STATE, "hot-key pre-aggregation needs the 1024-thread code pass");
                    } else
                        kfn = with_hash(hk, [&](auto h) {
                            constexpr int HK = decltype(h)::value;
                            return dpt == 4 ? reinterpret_cast<const void*>(&k_chunk_codes_pipe<BLOCK, ITEMS, HK, 4>)
                                 : dpt == 2 ? reinterpret_cast<const void*>(&k_chunk_codes_pipe<BLOCK, ITEMS, HK, 2>)
                                            : reinterpret_cast<const void*>(&k_chunk_codes_pipe<BLOCK, ITEMS, HK, 1>);
                        });
                }
            } else if (a.keys_only) {
                if constexpr (BLOCK == 512 && ITEMS == 8) {
                    if (a.nbins > BLOCK)
                        kfn = with_hash(hk, [&](auto h) {
                            constexpr int HK = decltype(h)::value;
                            return a.nbins > 2 * BLOCK ? reinterpret_cast<const void*>(&k_chunk_codes<BLOCK, ITEMS, HK, 4>)
                                                       : reinterpret_cast<const void*>(&k_chunk_codes<BLOCK, ITEMS, HK, 2>);
                        });
                }
                if (!kfn && a.nbins > BLOCK) return set_err(c, PHJ_ERR_INVALID, "keys-only pass 1: more digits than threads");
                if (!kfn)
                    kfn = with_hash(hk, [](auto h) {
                        return reinterpret_cast<const void*>(&k_chunk_codes<BLOCK, ITEMS, decltype(h)::value>);
                    });
            } else
                kfn = with_hash(hk, [](auto h) {
                    return reinterpret_cast<const void*>(&k_scatter_chunked<BLOCK, ITEMS, decltype(h)::value, 3, ROWS>);
                });
            if (c->p1_cols && !cols_form) return set_err(c, PHJ_ERR_STATE, "key column: this code pass has no column form");
            // workgroups per CU: what the LDS and the kernel's registers allow
            // (cached per kernel and LDS size; one cache per worker thread)
            const int occ = occupancy_or(kfn, kblock, lds, 1);
            const uint32_t fit = std::max<uint32_t>(1, std::min<uint32_t>(static_cast<uint32_t>(occ), static_cast<uint32_t>(160 * 1024 / lds)));
            uint32_t slots = std::max<uint32_t>(1, std::min<uint32_t>(per, fit * c->num_cus / a.nshards));
            // keys-only (the on-chip join): PHJ_P1_WPC2 half-workgroups per CU, not
            // every slot the LDS allows, so R's partition and tables on the aux
            // stream get CUs beside S's persistent pass 1 instead of queueing behind it
            if (a.keys_only && c->tune.p1_wpc2 > 0)
                slots = std::max<uint32_t>(
                    1, std::min<uint32_t>(per, std::min<uint32_t>(fit * 2, static_cast<uint32_t>(c->tune.p1_wpc2)) *
                                                   c->num_cus / (2 * a.nshards)));
            // (R's pass beside the hot-key prologue: CUs left to the prologue's workgroups)
            if (c->p1_free_cus > 0 && c->num_cus / a.nshards > c->p1_free_cus)
                slots = std::min<uint32_t>(slots, c->num_cus / a.nshards - c->p1_free_cus);
            if (c->tune.p1_slots > 0) slots = std::min<uint32_t>(per, c->tune.p1_slots);
            if (c->tune.p1_slots < 0) slots = per;   // one tile per workgroup
            PassArgs ak = a;
            const bool prof = PHJ_P1_PROF && pipe && kblock == 1024 && !is_r && (hot || !cols_form);   // (the forms pipe1024 builds with PROF)
            if (prof) {   // diagnostics (measurement build, PHJ_P1_PROF): synchronous, to stderr
                PHJ_TRY(ensure(c, c->cl_prof, 64 * 8));   // words 32.. (the LDS join's are 0..)
                ak.prof = static_cast<unsigned long long*>(c->cl_prof.p) + 32;
                PHJ_HIP(c, hipMemsetAsync(ak.prof, 0, kP1ProfWords * 8, c->ks));
            }
            void* kargs[] = {&ak, const_cast<uint32_t*>(&ntiles), const_cast<uint32_t*>(&per)};
            PHJ_TRY(launch_kernel(c, kfn, dim3(slots * a.nshards), dim3(kblock), kargs, lds, sname.c_str()));
            if (prof) {
                unsigned long long h[kP1ProfWords] = {};
                PHJ_HIP(c, hipMemcpyAsync(h, ak.prof, sizeof(h), hipMemcpyDeviceToHost, c->ks));
                PHJ_HIP(c, hipStreamSynchronize(c->ks));
                const double n = h[7] ? static_cast<double>(h[7]) : 1.0;
                if (h[15])   // the batched loop ran (the hot table on): its own phases
                    std::fprintf(stderr, "p1_prof %s grid %u batched: cycles per input tile: front %.0f append %.0f protocol+wait at A %.0f write %.0f sort stage %.0f (the PROF forms: 128 VGPRs, XXH3 spills 2); "
                                 "per batch: sort stage %.0f; tiles %llu batches %llu (%.3f per tile) iterations %llu\n",
                                 sname.c_str(), slots * a.nshards, h[0] / n, h[1] / n, h[2] / n, h[3] / n, h[4] / n,
                                 h[5] ? static_cast<double>(h[4]) / h[5] : 0.0, h[7], h[5], h[5] / n, h[14]);
                else
                std::fprintf(stderr, "p1_prof %s grid %u: cycles per tile: hash+rank %.0f B1 %.0f scan %.0f claims+B2 %.0f scatter+protocol %.0f B3 %.0f write %.0f; tiles %llu; "
                             "waves' max/mean B3->B1 %.0f/%.0f B1->B2 %.0f/%.0f B2->B3 %.0f/%.0f\n",
                             sname.c_str(), slots * a.nshards, h[0] / n, h[1] / n, h[2] / n, h[3] / n, h[4] / n, h[5] / n, h[6] / n, h[7],
                             h[8] / n, h[11] / n, h[9] / n, h[12] / n, h[10] / n, h[13] / n);
            }
        } else {
            (void)grid;
            return set_err(c, PHJ_ERR_INVALID, "chunked pass 1 needs AoS input and output, <= 8 tuples per thread");
        }
        return timer_end(c);
    }
    // algorithmic bytes: the histogram reads the key (a whole 16-B tuple when AoS)
    // or 1-2 B of a digit column; the scatter reads and writes every tuple once
    // (16 + 16 B) plus the digit column it leaves for pass 2
    const uint64_t hbytes = a.in_dig ? n * (a.dig_wide ? 2 : 1) : n * (IN_AOS ? 16 : 8) - n * kcol;
    PHJ_TRY(timer_begin(c, hname.c_str(), hbytes));
    if (a.in_dig) {
        // wave per tile: 4 tiles per workgroup
        PassArgs ac = a;
        uint32_t cgrid = (grid + 3) / 4;
        cgrid = (cgrid + 7) & ~7u;
        const size_t clds = 4ull * a.nbins * 4;
        if (a.dig_wide)
            hipLaunchKernelGGL((k_hist_col<T, uint16_t>), dim3(cgrid), dim3(256), clds, c->ks, ac);
        else
            hipLaunchKernelGGL((k_hist_col<T, uint8_t>), dim3(cgrid), dim3(256), clds, c->ks, ac);
    } else
        with_hash(hk, [&](auto h) {
            if constexpr (ROWS == 1)
                hipLaunchKernelGGL((k_hist<BLOCK, ITEMS, false, decltype(h)::value, true>), dim3(grid), dim3(BLOCK), hist_lds, c->ks, a);
            else   // (ROWS 2: the tuple form already reads the ids alone)
                hipLaunchKernelGGL((k_hist<BLOCK, ITEMS, IN_AOS, decltype(h)::value>), dim3(grid), dim3(BLOCK), hist_lds, c->ks, a);
        });
    PHJ_LAUNCHED(c, hname);
    PHJ_TRY(timer_end(c));
    PHJ_TRY(timer_begin(c, cname.c_str(), static_cast<uint64_t>(hist_len) * 12));
    PHJ_TRY(scan_u32(c, a.hist, hist_len, 1, hist_len, c->scan_scratch));
    PHJ_TRY(timer_end(c));
    PHJ_TRY(timer_begin(c, sname.c_str(), n * 32 - n * kcol + (a.out_dig ? n * (a.dig_wide ? 2 : 1) : 0)));
    with_hash(hk, [&](auto h) {
        hipLaunchKernelGGL((k_scatter<BLOCK, ITEMS, IN_AOS, OUT_AOS, decltype(h)::value, ROWS>), dim3(grid), dim3(BLOCK), sc_lds, c->ks, a);
    });
    PHJ_LAUNCHED(c, sname);
    PHJ_TRY(timer_end(c));
    return PHJ_OK;
}

// Workgroup size and tile of the tile kernels: the tuned shape when it is one
// of the compiled ones and its scatter fits the LDS, else 512 x 4096.
struct TileShape {
    int block, tile;
};

TileShape tile_shape(const phj_ctx* c, uint32_t nb) {
    const int b = c->tune.block, t = c->tune.tile;
    const bool compiled = (b == 256 && (t == 2048 || t == 4096)) || (b == 512 && (t == 2048 || t == 4096 || t == 8192)) ||
                          (b == 1024 && t == 8192);
    if (compiled && scatter_lds_bytes(t, nb, b / 64) <= 160 * 1024) return TileShape{b, t};
    return TileShape{512, 4096};
}

// One partition pass over `ntiles` tiles (an upper bound for segmented passes).
// rows: launch_pass_t's ROWS (pass 1 over the bound relation only).
int launch_pass(phj_ctx* c, int hk, bool in_aos, bool out_aos, PassArgs a, uint32_t ntiles,
                const std::string& prefix, uint64_t n, uint32_t hist_len, int rows = 0) {
    if (ntiles == 0) return PHJ_OK;
    uint32_t grid = ntiles;
    grid = (ntiles + 7) & ~7u;
    a.xcd_remap = 1;
    const TileShape sh = tile_shape(c, a.nbins);
    const int io = (in_aos ? 2 : 0) + (out_aos ? 1 : 0);
    if (rows < 0 || rows > 2 || (rows != 0 && !in_aos)) return set_err(c, PHJ_ERR_INVALID, "unsupported pass layout");
#define PHJ_PASS_CASES(B, I)                                                        \
    switch (io + 4 * rows) {   /* (one statement: it follows an unbraced if) */     \
        case 4 + 2: return launch_pass_t<B, I, true, false, 1>(c, hk, a, grid, prefix, n, hist_len); \
        case 4 + 3: return launch_pass_t<B, I, true, true, 1>(c, hk, a, grid, prefix, n, hist_len);  \
        case 8 + 2: return launch_pass_t<B, I, true, false, 2>(c, hk, a, grid, prefix, n, hist_len); \
        case 8 + 3: return launch_pass_t<B, I, true, true, 2>(c, hk, a, grid, prefix, n, hist_len);  \
        case 0: return launch_pass_t<B, I, false, false>(c, hk, a, grid, prefix, n, hist_len); \
        case 2: return launch_pass_t<B, I, true, false>(c, hk, a, grid, prefix, n, hist_len);  \
        case 3: return launch_pass_t<B, I, true, true>(c, hk, a, grid, prefix, n, hist_len);   \
        default: return set_err(c, PHJ_ERR_INVALID, "unsupported pass layout");     \
    }
    a.nt_store = 0;
    // nontemporal tuple loads: 1 = the chunked pass 1 only (the relation is read
    // once there; the stable pass 1 re-reads it after its histogram, and at
    // 25-100M tuples that re-read is measured 0.01-0.02 ms slower with them),
    // 2 = every pass
    a.nt_load = (c->tune.nt_load == 2 || (c->tune.nt_load == 1 && a.chunk_cursor != nullptr && prefix.size() >= 3 &&
                                         prefix.compare(prefix.size() - 3, 3, ".p1") == 0)) ? 1u : 0u;
    if (sh.block == 256 && sh.tile == 2048) PHJ_PASS_CASES(256, 8)
    if (sh.block == 256 && sh.tile == 4096) PHJ_PASS_CASES(256, 16)
    if (sh.block == 512 && sh.tile == 2048) PHJ_PASS_CASES(512, 4)
    if (sh.block == 512 && sh.tile == 8192) PHJ_PASS_CASES(512, 16)
    if (sh.block == 1024 && sh.tile == 8192) PHJ_PASS_CASES(1024, 8)
    PHJ_PASS_CASES(512, 8)
#undef PHJ_PASS_CASES
}

// Whether partition_state takes the chunked pass 1 for n tuples under plan pl
// (ko: the keys-only code form of the counting joins). Chunked pass 1
// (unordered partitions, tile kernels): pass-1 chunks are the pass-2 tiles,
// every digit's run of a tile fits one workgroup thread (nb1 <= block) and
// spans at most two chunks (tile1 == tile2), and every pool slot of the
// shards' pools is a uint32 (the pool bound below).
// Measured: it pays at 200M tuples (16 chains per digit) and
// loses to the stable pass below ~100M, where fewer shards (more
// workgroups per cursor line) or more partial chunks cost more than the
// histogram read saves; so it starts at p1_min_tiles tiles. The keys-only
// form for the on-chip probe (half the bytes, three workgroups per CU)
// wins at every size measured (25M-200M), with shards of p1_ko_tps tiles.
// use_cluster asks the same of the probe side (the LDS join needs S's codes).
bool chunked_pass1(const phj_ctx* c, const Plan& pl, uint64_t n64, bool ko) {
    if (pl.npass != 2 || pl.stable || !c->tune.p1_chunk || n64 == 0 || n64 >= (1ull << 32) - 2 * 4096) return false;
    const uint64_t n = n64;
    const TileShape sh = tile_shape(c, pl.nb1);
    const uint32_t tile = sh.tile;
    if (tile != tile_shape(c, pl.nb2).tile) return false;
    if (!ko && (n + tile - 1) / tile < static_cast<uint64_t>(c->tune.p1_min_tiles)) return false;
    if (pl.nb1 > static_cast<uint32_t>(sh.block) * (ko && sh.block == 512 && tile == 4096 ? 4u : 1u)) return false;
    if (tile / sh.block > 8) return false;   // registers: the next tile is prefetched
    if ((3 * (n / tile + kShards) + kShards * pl.nb1) * tile >= (1ull << 32)) return false;
    const bool pipe = ko && c->tune.p1_pipe && sh.block == 512 && tile == 4096;
    // the pipelined code pass's pool (pipe_pool_stride per shard)
    if (pipe && ((kPipeRes + 1) * (n / tile + kShards) + kShards * (3ull * pl.nb1 + 1)) * tile >= (1ull << 32)) return false;
    return true;
}

// A side bound as columns whose keys-only pass 1 under plan pl is the 1024 x 4
// pipelined code pass with one digit per thread (the counting LDS join's
// default schedule): that pass, and the hot-key sample, read the key column
// itself (k_chunk_codes_pipe COLS, k_hot_sample COLS) and no tuple copy is
// made. Every other pass runs on the packed copy (need_tuples).
bool cols_native(const phj_ctx* c, const SideState& S, const Plan& pl, bool is_r) {
    if (!S.columns || S.n == 0) return false;
    if (!c->tune.p1_pipe || c->tune.p1_block != 1024 || pl.nb1 > 1024 || (is_r && !c->tune.r_chunk)) return false;
    const TileShape sh = tile_shape(c, pl.nb1);
    return sh.block == 512 && sh.tile == 4096 && chunked_pass1(c, pl, S.n, true);
}

// Where pass 1 takes the payload it moves from: the bound payloads, or (the
// row-number joins, phj_index.h) the tuple's position in the relation as
// bound. The second form reads nothing but keys: the key column of a columnar
// binding (even beside a packed copy: half the bytes), or the ids of the
// tuples, and needs no packed copy.
enum class PaySrc { Bound, RowNumber };

int partition_state(phj_ctx* c, SideState& S, const char* tag, const Plan& pl, bool p1_only,
                    unsigned long long* zero = nullptr, uint32_t max_shards = kShards, PaySrc pay = PaySrc::Bound) {
    c->scan_scratch = &S.partials;
    if (!S.rel && !S.columns && S.n > 0) return set_err(c, PHJ_ERR_STATE, "relation not bound");
    const int rows = pay == PaySrc::Bound ? 0 : S.columns ? 1 : 2;   // launch_pass_t's ROWS
    if (rows && p1_only) return set_err(c, PHJ_ERR_INVALID, "row numbers: whole tuples are partitioned");
    const bool cols = p1_only && cols_native(c, S, pl, &S == &c->side[PHJ_SIDE_BUILD]);
    if (!S.rel && !cols && !rows && !c->dry && S.n > 0) return set_err(c, PHJ_ERR_STATE, "relation bound as columns: no tuple copy was packed for this pass");
    const uint64_t n64 = S.n;
    if (n64 >= (1ull << 32) - 2 * 4096) return set_err(c, PHJ_ERR_RANGE, "relation above 2^32 tuples per device");
    const uint32_t n = static_cast<uint32_t>(n64);
    const uint32_t tile = tile_shape(c, pl.nb1).tile;
    const uint32_t tile2 = pl.npass == 2 ? tile_shape(c, pl.nb2).tile : 0;
    const uint32_t nt1 = (n + tile - 1) / tile;
    const bool p1_aos = pl.npass == 2;
    // pass 1 leaves the pass-2 digit in a column (tile kernels only)
    // (p1_only: the probe re-hashes the keys itself, nothing reads the column)
    const bool dcol = pl.npass == 2 && !p1_only;
    const uint32_t dbytes = pl.bits2 > 8 ? 2 : 1;
    // Chunked pass 1 (unordered partitions, tile kernels): pass-1 chunks are
    // the pass-2 tiles, every digit's run of a tile fits one workgroup thread
    // (nb1 <= block) and spans at most two chunks (tile1 == tile2).
    // Measured: it pays at 200M tuples (16 chains per digit) and
    // loses to the stable pass below ~100M, where fewer shards (more
    // workgroups per cursor line) or more partial chunks cost more than the
    // histogram read saves; so it starts at p1_min_tiles tiles. The keys-only
    // form for the on-chip probe (half the bytes, three workgroups per CU)
    // wins at every size measured (25M-200M), with shards of p1_ko_tps tiles.
    const bool ko = p1_only;
    const bool chunked = chunked_pass1(c, pl, n64, ko);
    S.hcoded = chunked && ko;   // k_chunk_codes
    // chains per digit: ~kTilesPerShard tiles each, a power of two <= kShards
    // (max_shards < kShards: R in tile mode takes exactly that many, so a
    // cluster below the LDS limit has at most max_shards + lim / tile runs)
    uint32_t nshards = 1;
    const uint32_t tps = max_shards < kShards ? std::max<uint32_t>(1, (nt1 + max_shards - 1) / max_shards)
                                              : static_cast<uint32_t>(ko ? c->tune.p1_ko_tps : c->tune.p1_tps);
    while (nshards < max_shards && static_cast<uint64_t>(nshards) * tps < nt1) nshards <<= 1;
    // pool of pass-1 chunks, one region per shard: a shard takes at most
    // `per` tiles, each with two chunks reserved up front (k_scatter_chunked, k_chunk_codes;
    // unused ones are never touched), then at most per + nb1 chunks for its
    // chains' other starts (each chain wastes at most one partial chunk)
    const uint32_t per = (nt1 + nshards - 1) / nshards;
    // (the pipelined code pass: 2 static chunks per chain, kPipeRes per tile, then its counter)
    const bool pipe = ko && c->tune.p1_pipe && tile_shape(c, pl.nb1).block == 512 && tile == 4096;
    const uint32_t pool_stride = pipe ? pipe_pool_stride(per, pl.nb1) : 3 * per + pl.nb1;
    const uint32_t maxch = per + 1;   // chunks of one chain (every tuple of a shard in one digit)
    const size_t slots1 = chunked ? static_cast<size_t>(nshards) * pool_stride * tile : n;
    // pass-2 tiles (bound): one partial tile per segment, or per chain when chunked
    const uint32_t nt2 = pl.npass != 2 ? 0 : (n + tile2 - 1) / tile2 + pl.nb1 * (chunked ? nshards : 1);
    const uint32_t nt2max = nt2 + 8;
    // workspace (grow-only; allocation is outside the timed phases on reuse)
    PHJ_TRY(ensure(c, S.kA, slots1 * (p1_aos ? 16 : 8)));
    if (!p1_aos) PHJ_TRY(ensure(c, S.pA, static_cast<size_t>(n) * 8));
    if (!chunked) PHJ_TRY(ensure(c, S.hist1, static_cast<size_t>(nt1) * pl.nb1 * 4));
    PHJ_TRY(ensure(c, S.bounds1, (static_cast<size_t>(pl.nb1) + 1) * 4));
    if (pl.npass == 2) {
        PHJ_TRY(ensure(c, S.kB, static_cast<size_t>(n) * 8));
        PHJ_TRY(ensure(c, S.pB, static_cast<size_t>(n) * 8));
        PHJ_TRY(ensure(c, S.tbase2, (static_cast<size_t>(pl.nb1) + 1) * 4));
        PHJ_TRY(ensure(c, S.hist2, (static_cast<size_t>(nt2) + 8) * pl.nb2 * 4));
        PHJ_TRY(ensure(c, S.tseg2, (static_cast<size_t>(nt2) + 8) * 4));
        PHJ_TRY(ensure(c, S.bounds, (static_cast<size_t>(pl.Ppad) + 1) * 4));
        if (dcol) PHJ_TRY(ensure(c, S.dig, slots1 * dbytes + 64));
    }
    if (chunked) {
        PHJ_TRY(ensure(c, S.ccur, chunk_state_bytes(pl.nb1)));
        if (ko) PHJ_TRY(ensure(c, S.csink, static_cast<size_t>(kSinkGroups) * std::max(1024, tile_shape(c, pl.nb1).block) * 8));
        PHJ_TRY(ensure(c, S.tstart, static_cast<size_t>(nt2max) * 8));   // tile_start, tile_cnt
        // all zero between passes (kPublished): cleared when new, and when a
        // pass that published entries never reached k_tile_chunks (an error)
        // (a reallocation can return the same address: compare the size)
        const size_t before = S.ctab.bytes;
        PHJ_TRY(ensure(c, S.ctab, static_cast<size_t>(nshards) * pl.nb1 * maxch * 8));
        if (S.ctab.bytes != before) S.ctab_dirty = true;
        if (S.ctab_dirty && !c->dry) {
            PHJ_HIP(c, hipMemsetAsync(S.ctab.p, 0, S.ctab.bytes, c->ks));
            S.ctab_dirty = false;
        }
    }
    if (c->dry) {   // scan scratch of both passes, then nothing is launched
        if (!chunked) PHJ_TRY(scan_u32(c, nullptr, nt1 * pl.nb1, 1, nt1 * pl.nb1, c->scan_scratch));
        if (pl.npass == 2 && n) PHJ_TRY(scan_u32(c, nullptr, nt2 * pl.nb2, 1, nt2 * pl.nb2, c->scan_scratch));
        return PHJ_OK;
    }
    // pass 1: AoS relation -> SoA columns A (cols: the key column -> codes)
    PassArgs a{};
    a.in_keys = cols || rows == 1 ? S.ckeys : reinterpret_cast<const int64_t*>(S.rel);
    a.out_keys = static_cast<int64_t*>(S.kA.p);
    a.out_pays = static_cast<int64_t*>(S.pA.p);
    a.hist = static_cast<uint32_t*>(S.hist1.p);
    a.seg_bounds = nullptr;
    a.tile_base = nullptr;
    a.nseg = 1;
    a.n = n;
    a.ntiles1 = nt1;
    a.nbins = pl.nb1;
    a.nbits = pl.bits1;
    a.f = digit_fn(pl, 1);
    if (dcol) {
        a.out_dig = S.dig.p;
        a.dig_wide = dbytes == 2 ? 1u : 0u;
        a.dig2_mask = pl.dmask2;
    }
    if (chunked) {
        // the counting probe consumes pass 1 on chip and reads only keys
        a.keys_only = ko ? 1u : 0u;
        a.chunk_cursor = static_cast<uint32_t*>(S.ccur.p);
        a.sink = static_cast<unsigned long long*>(S.csink.p);
        a.chunk_tab = static_cast<unsigned long long*>(S.ctab.p);
        a.maxch = maxch;
        a.pool_stride = pool_stride;
        a.nshards = nshards;
        S.ctab_dirty = n > 0;   // until k_tile_chunks has cleared what pass 1 publishes
        S.chunk_check = n > 0;
    }
    unsigned long long* kept = nullptr;   // S's pre-aggregating pass: the tuples it wrote
    if (c->hot_on && &S == &c->side[PHJ_SIDE_PROBE]) {   // phj_join's counting LDS join, default schedule (hot_begin): S's pass
        if (!S.hcoded) return set_err(c, PHJ_ERR_STATE, "hot-key pre-aggregation needs the chunked code pass");
        uint32_t* st = static_cast<uint32_t*>(c->hot.p);
        a.hot_code = reinterpret_cast<const unsigned long long*>(st + kHotCounters);
        a.hot_w = reinterpret_cast<unsigned long long*>(st + kHotCounters) + static_cast<size_t>(pl.nb1) * kHotPer;
        a.hot_ctl = reinterpret_cast<const uint32_t*>(a.hot_w + static_cast<size_t>(pl.nb1) * kHotPer);
        a.hot_min_mass = c->hot_min_mass;
        kept = reinterpret_cast<unsigned long long*>(const_cast<uint32_t*>(a.hot_ctl) + 2);
    }
    uint32_t* tb2 = pl.npass == 2 ? static_cast<uint32_t*>(S.tbase2.p) : nullptr;
    c->p1_cols = cols;
    const int rc1 = launch_pass(c, pl.hk, true, p1_aos, a, nt1, std::string(tag) + ".p1", n, nt1 * pl.nb1, rows);
    c->p1_cols = false;
    PHJ_TRY(rc1);
    if (chunked) {
        uint4* clr = nullptr;   // another pass's chunk state, cleared here (c->p1_clear)
        if (c->p1_clear) {
            clr = static_cast<uint4*>(c->p1_clear);
            c->p1_cleared = c->p1_clear;
            c->p1_clear = nullptr;
        }
        {
            hipLaunchKernelGGL(k_pass1_finish_sizes, dim3(1), dim3(kFinSizesBlock), 0, c->ks, a.chunk_cursor, pl.nb1, nshards, n, tile2,
                               static_cast<uint32_t*>(S.bounds1.p), tb2, zero, clr, static_cast<uint32_t>(c->p1_clear_bytes / 16), kept);
            PHJ_LAUNCHED(c, "k_pass1_finish_sizes");
        }
    } else {
        hipLaunchKernelGGL(k_pass1_finish, dim3(1), dim3(kFinBlock), 0, c->ks, a.hist, nt1, pl.nb1, n,
                           pl.npass == 2 ? tile2 : tile, static_cast<uint32_t*>(S.bounds1.p), tb2);
        PHJ_LAUNCHED(c, "k_pass1_finish");
    }
    if (pl.npass == 1) {
        S.view.keys = static_cast<const int64_t*>(S.kA.p);
        S.view.payloads = static_cast<const int64_t*>(S.pA.p);
        S.view.bounds = static_cast<const uint32_t*>(S.bounds1.p);
    } else {
        PassArgs b{};
        b.in_keys = static_cast<const int64_t*>(S.kA.p);
        b.in_pays = p1_aos ? nullptr : static_cast<const int64_t*>(S.pA.p);
        b.out_keys = static_cast<int64_t*>(S.kB.p);
        b.out_pays = static_cast<int64_t*>(S.pB.p);
        b.hist = static_cast<uint32_t*>(S.hist2.p);
        b.seg_bounds = static_cast<const uint32_t*>(S.bounds1.p);
        b.tile_base = tb2;
        b.tile_seg = static_cast<const uint32_t*>(S.tseg2.p);
        b.nseg = pl.nb1;
        b.keys_only = a.keys_only;
        if (n) {
            if (chunked) {
                uint32_t* ts = static_cast<uint32_t*>(S.tstart.p);
                uint32_t* tc = ts + nt2max;
                {
                    hipLaunchKernelGGL(k_tile_chunks, dim3((pl.nb1 * nshards + kWaves - 1) / kWaves), dim3(kBlock), 0, c->ks, tb2,
                                       static_cast<uint32_t*>(S.ccur.p), pl.nb1, nshards,
                                       static_cast<unsigned long long*>(S.ctab.p), maxch, pool_stride, tile2,
                                       static_cast<uint32_t*>(S.tseg2.p), ts, tc);
                    PHJ_LAUNCHED(c, "k_tile_chunks");
                }
                S.ctab_dirty = false;
                b.tile_start = ts;
                b.tile_cnt = tc;
            } else {   // stable layout: tile -> digit
                hipLaunchKernelGGL(k_tile_seg, dim3((pl.nb1 + kWaves - 1) / kWaves), dim3(kBlock), 0, c->ks, tb2,
                                   pl.nb1, static_cast<uint32_t*>(S.tseg2.p));
                PHJ_LAUNCHED(c, "k_tile_seg");
            }
        }
        b.n = n;
        b.ntiles1 = 0;
        b.nbins = pl.nb2;
        b.nbits = pl.bits2;
        b.f = digit_fn(pl, 2);
        if (dcol) {
            b.in_dig = S.dig.p;
            b.dig_wide = dbytes == 2 ? 1u : 0u;
        }
        const uint32_t grid2 = n ? nt2 : 0;
        if (p1_only) {   // the caller consumes the pass-2 tiles itself (k_probe_ht)
            S.p2 = b;
            S.nt2 = grid2;
            S.view = phj_partitioned{};
            S.partitioned = false;
            S.plan = pl;
            return PHJ_OK;
        }
        PHJ_TRY(launch_pass(c, pl.hk, p1_aos, false, b, grid2, std::string(tag) + ".p2", n, grid2 * pl.nb2));
        const uint32_t nbnd = pl.Ppad + 1;
        hipLaunchKernelGGL(k_pass2_bounds, dim3((nbnd + kBlock - 1) / kBlock), dim3(kBlock), 0, c->ks,
                           b.hist, tb2, b.seg_bounds, pl.nb1, pl.nb2, n, static_cast<uint32_t*>(S.bounds.p));
        PHJ_LAUNCHED(c, "k_pass2_bounds");
        S.view.keys = static_cast<const int64_t*>(S.kB.p);
        S.view.payloads = static_cast<const int64_t*>(S.pB.p);
        S.view.bounds = static_cast<const uint32_t*>(S.bounds.p);
    }
    S.view.n = n;
    S.view.num_partitions = pl.Ppad;
    S.partitioned = true;
    S.plan = pl;
    return PHJ_OK;
}

// zero: a word the pass-1 bookkeeping clears (the on-chip probe's count),
// or null
int partition_side(phj_ctx* c, int s, const Plan& pl, bool p1_only = false, unsigned long long* zero = nullptr,
                   PaySrc pay = PaySrc::Bound) {
    return partition_state(c, c->side[s], s == PHJ_SIDE_BUILD ? "R" : "S", pl, p1_only, zero, kShards, pay);
}

// Hot-key pre-aggregation (phj_hot.h) for phj_join's counting LDS join in its
// default schedule (PHJ_R_ORDER=1, R in tile mode): whether this join takes
// it. A host-side decision: both code passes must be the 1024 x 4 pipelined
// form with one digit per thread (the LDS holds the table beside S's pass's
// own 90 KB up to 1024 clusters), R's tile list must be the one the LDS join
// reads (it resolves the hot weights), and S must be large enough that the sample
// (kHotTiles tiles, two reads) is small against its pass: 32 times the sample.
constexpr uint64_t kHotMinS = 32ull * kHotTiles * kHotTile;   // 16.8M tuples
bool hot_wanted(const phj_ctx* c, const Plan& cpl, uint64_t nS, uint64_t nR) {
    if (!PHJ_PREAGG || c->hot_mode == 1 || c->dry || nS == 0) return false;
    if (c->tune.r_order != 1 || !c->tune.r_chunk || !c->tune.p1_pipe || c->tune.p1_block != 1024) return false;
    const TileShape sh = tile_shape(c, cpl.nb1);
    if (sh.block != 512 || sh.tile != 4096 || cpl.nb1 > 1024) return false;
    if (!chunked_pass1(c, cpl, nS, true) || (nR > 0 && !chunked_pass1(c, cpl, nR, true))) return false;
    if (cluster_empty0(cpl) == 0) return false;   // one cluster: no code marks an empty way
    return c->hot_mode == 2 || nS >= kHotMinS;
}

// The sample and the selection, on the main stream before S's pass 1; S's
// code pass of this join then takes its HOT form (c->hot_on). Forced
// mode (phj_debug_preagg) takes the lowest threshold and any coverage.
int hot_begin(phj_ctx* c, const Plan& cpl, const SideState& S) {
    const bool cols = cols_native(c, S, cpl, false);   // the sample reads the key column
    PHJ_TRY(ensure(c, c->hot, hot_state_bytes(cpl.nb1)));
    const bool forced = c->hot_mode == 2;
    HotArgs h{};
    h.rel = cols ? S.ckeys : reinterpret_cast<const int64_t*>(S.rel);
    h.n = static_cast<uint32_t>(S.n);
    h.ntiles = (h.n + kHotTile - 1) / kHotTile;
    h.nsamp = std::min(kHotTiles, h.ntiles);
    h.thr = forced ? 2u : std::max(2u, kHotThreshold * h.nsamp / kHotTiles);
    h.f = digit_fn(cpl, 1);
    h.nb = cpl.nb1;
    h.e0 = cluster_empty0(cpl);
    h.counters = static_cast<uint32_t*>(c->hot.p);
    h.code = reinterpret_cast<unsigned long long*>(h.counters + kHotCounters);
    h.w = h.code + static_cast<size_t>(cpl.nb1) * kHotPer;
    h.ctl = reinterpret_cast<uint32_t*>(h.w + static_cast<size_t>(cpl.nb1) * kHotPer);
    h.rep = reinterpret_cast<unsigned long long*>(h.ctl + kHotCtlWords);
    // a table covering under an eighth of the sample is ignored by S's pass and the LDS join
    c->hot_min_mass = forced ? 0u : static_cast<uint32_t>(std::min<uint64_t>(S.n, static_cast<uint64_t>(h.nsamp) * kHotTile) / 8);
    c->hot_n = S.n;
    // no timer events under PHJ_LEAN_TIMERS (each one between two kernels costs ~4 us)
    const bool timed = !c->lean_timers;
    if (timed) PHJ_TRY(timer_begin(c, "S.hot", 1ull * h.nsamp * kHotTile * (cols ? 8 : 16)));
    const void* ksample = with_hash(cpl.hk, [&](auto hh) {
        constexpr int HK = decltype(hh)::value;
        return cols ? reinterpret_cast<const void*>(&k_hot_sample<HK, true>) : reinterpret_cast<const void*>(&k_hot_sample<HK>);
    });
    // auto mode: a sample workgroup whose own tiles show no skew writes nothing
    h.staged = !forced && h.nsamp == kHotTiles ? 1u : 0u;
    // the counters and control words: left zero by the last join's selection,
    // unless this is another buffer or layout, or that selection did not run
    // (hot_clean is set again once this join's has been launched, and dropped
    // by a join that fails)
    const bool clean = c->hot_clean == c->hot.p && c->hot_clean_nb == cpl.nb1;
    c->hot_clean = nullptr;
    if (!clean) {
        hipLaunchKernelGGL(k_hot_clear, dim3(16), dim3(kHotBlock), 0, c->ks, h);
        PHJ_LAUNCHED(c, "k_hot_clear");
    }
    void* sargs[] = {&h};
    // (kHotTilesPerWg sample tiles per workgroup, one workgroup of selection:
    // at most 32 workgroups at a time, so R's pass 1 can run beside them)
    const uint32_t wide = (h.nsamp + kHotTilesPerWg - 1) / kHotTilesPerWg;
    PHJ_TRY(launch_kernel(c, ksample, dim3(wide), dim3(kHotBlock), sargs, kHotCounters * 2, "k_hot_sample"));
    hipLaunchKernelGGL(k_hot_select, dim3(1), dim3(kHotBlock), hot_select_lds_bytes(cpl.nb1), c->ks, h);
    PHJ_LAUNCHED(c, "k_hot_select");
    c->hot_clean = c->hot.p;
    c->hot_clean_nb = cpl.nb1;
    if (timed) PHJ_TRY(timer_end(c));
    c->hot_on = true;
    c->hot_ran = true;
    return PHJ_OK;
}

// Build over `nseg` partitioned build segments and probe the ctx's partitioned
// probe side. Records "build" and "probe" timers; returns events bracketing them.
int build_and_probe(phj_ctx* c, const Plan& pl, int nseg, const phj_partitioned* segs,
                    hipEvent_t* e_build0, hipEvent_t* e_build1, hipEvent_t* e_probe1) {
    SideState& PS = c->side[PHJ_SIDE_PROBE];
    if (!c->dry && (!PS.partitioned || !(PS.plan == pl)))
        return set_err(c, PHJ_ERR_STATE, "probe relation not partitioned with these params");
    if (nseg < 1 || nseg > kMaxSegs) return set_err(c, PHJ_ERR_INVALID, "nbuild must be in [1,16]");
    const uint32_t P = pl.Ppad;
    SegList L{};
    L.nseg = static_cast<uint32_t>(nseg);
    L.P = P;
    uint64_t nR = 0;
    for (int g = 0; g < nseg; g++) {
        if (segs[g].num_partitions != P)
            return set_err(c, PHJ_ERR_INVALID, "build segment partition count mismatch");
        L.seg[g].keys = segs[g].keys;
        L.seg[g].pays = segs[g].payloads;
        if ((segs[g].payloads == nullptr) != (segs[0].payloads == nullptr))
            return set_err(c, PHJ_ERR_INVALID, "build segments must all carry payloads or none");
        L.seg[g].bounds = segs[g].bounds;
        nR += segs[g].n;
    }
    if (nR >= (1ull << 32) - 1) return set_err(c, PHJ_ERR_RANGE, "build side above 2^32 tuples");
    const uint64_t nS = c->dry ? PS.n : PS.view.n;
    // fused when the average partition fits one LDS round with margin (larger
    // ones take extra rounds, each re-probing the item's S keys)
    if (!pl.chained && c->tune.fused && (nR + P - 1) / P * 3 <= static_cast<uint64_t>(kFusedTcap) * 2) {
        // fused per-partition join with LDS tables: HashJoin.hpp:267-303
        const size_t nslots = nS / kFusedChunk + P + 1;
        PHJ_TRY(ensure(c, c->fitems, nslots * sizeof(FusedItem)));
        PHJ_TRY(ensure(c, c->count, 32));
        if (!c->split.p) {
            PHJ_TRY(ensure(c, c->split, 16));
            PHJ_HIP(c, hipMemsetAsync(c->split.p, 0, 16, c->ks));
        }
        if (c->dry) return PHJ_OK;
        PHJ_HIP(c, hipMemsetAsync(c->count.p, 0, 8, c->ks));
        PHJ_TRY(mark(c, e_build0));
        // algorithmic bytes: R keys once (build), S keys once (probe)
        PHJ_TRY(timer_begin_split(c, nR * 8, nS * 8));
        hipLaunchKernelGGL(k_fused_items, dim3((P + kWaves - 1) / kWaves), dim3(kBlock), 0, c->ks,
                           PS.view.bounds, P, static_cast<FusedItem*>(c->fitems.p));
        PHJ_LAUNCHED(c, "k_fused_items");
        FusedArgs fa{};
        fa.L = L;
        fa.skeys = PS.view.keys;
        fa.sbounds = PS.view.bounds;
        fa.items = static_cast<const FusedItem*>(c->fitems.p);
        fa.nitems = static_cast<uint32_t>(nslots - 1);
        fa.count = static_cast<unsigned long long*>(c->count.p);
        fa.cycles = static_cast<unsigned long long*>(c->split.p);
        fa.seed = pl.seed;
        const void* kfn = with_hash(pl.hk, [](auto h) {
            return reinterpret_cast<const void*>(&k_join_fused<decltype(h)::value, kFusedKPL, kFusedTcap>);
        });
        const uint32_t grid = chip_grid(c, (nslots + kWaves - 1) / kWaves, occupancy_or(kfn, kBlock, 0, 2));
        void* kargs[] = {&fa};
        PHJ_HIP(c, hipLaunchKernel(kfn, dim3(grid), dim3(kBlock), kargs, 0, c->ks));
        PHJ_LAUNCHED(c, "k_join_fused");
        PHJ_TRY(timer_end_split(c));
        PHJ_TRY(mark(c, e_probe1));
        *e_build1 = *e_probe1;
        c->last_fused = true;
        return PHJ_OK;
    }
    c->last_fused = false;
    // very large partitions (the reference's -p 32 .. 128 at 10M build tuples):
    // partitioned bucket tables, whose build is one pass of atomics over all
    // tuples; the CSR build below gives each partition one workgroup (3.9 ms at
    // -p 32 against 0.76), while its probe is faster from -p 1024 up
    if (!pl.chained && (c->tune.ptab > 1 || (c->tune.ptab == 1 && (nR + P - 1) / P >= 65536))) {
        // partitioned bucket tables in HBM (large partitions)
        const uint32_t ratio_x256 = static_cast<uint32_t>(kNPDefaultRatio * 256);
        const size_t nbk_bound = static_cast<size_t>(nR) * ratio_x256 / 256 / kNPSlots + 2 * static_cast<size_t>(P) + 1;
        PHJ_TRY(ensure(c, c->np_tab, nbk_bound * sizeof(NPBucket)));
        PHJ_TRY(ensure(c, c->np_pays, nbk_bound * kNPSlots * 8));
        PHJ_TRY(ensure(c, c->prep, (static_cast<size_t>(P) + 1) * 4));
        PHJ_TRY(ensure(c, c->count, 32));
        PtabArgs ta{};
        ta.L = L;
        uint64_t off = 0;
        for (int g = 0; g < nseg; g++) {
            ta.segoff[g] = static_cast<uint32_t>(off);
            off += segs[g].n;
        }
        ta.segoff[nseg] = static_cast<uint32_t>(off);
        ta.tab = static_cast<NPBucket*>(c->np_tab.p);
        ta.pays = static_cast<int64_t*>(c->np_pays.p);
        ta.tob = static_cast<const uint32_t*>(c->prep.p);
        ta.f = DigitFn{pl.seed, pl.P, pl.mode == 1 ? (~0ull) / pl.P : 0, pl.mode, 0, 0xffffffffu,
                       pl.sub_bits, pl.sub_shift, 0};
        ta.seed = pl.seed;
        if (c->dry) return scan_u32(c, nullptr, P + 1, 1, P + 1);
        PHJ_TRY(mark(c, e_build0));
        PHJ_TRY(timer_begin(c, "build", nR * 32 + nbk_bound * 64));
        PHJ_HIP(c, hipMemsetAsync(c->np_tab.p, 0, nbk_bound * sizeof(NPBucket), c->ks));
        hipLaunchKernelGGL(k_pt_prep, dim3((P + 1 + kBlock - 1) / kBlock), dim3(kBlock), 0, c->ks, L, ratio_x256,
                           static_cast<uint32_t*>(c->prep.p));
        PHJ_LAUNCHED(c, "k_pt_prep");
        PHJ_TRY(scan_u32(c, static_cast<uint32_t*>(c->prep.p), P + 1, 1, P + 1));
        if (nR) {
            const dim3 bg(static_cast<uint32_t>((nR + kBlock - 1) / kBlock));
            with_hash(pl.hk, [&](auto h) {
                hipLaunchKernelGGL((k_pt_build<decltype(h)::value>), bg, dim3(kBlock), 0, c->ks, ta);
            });
            PHJ_LAUNCHED(c, "k_pt_build");
        }
        PHJ_TRY(timer_end(c));
        PHJ_TRY(mark(c, e_build1));
        PHJ_HIP(c, hipMemsetAsync(c->count.p, 0, 8, c->ks));
        PHJ_TRY(timer_begin(c, "probe", nS * 8 + nS * 64));
        if (nS) {
            constexpr int IT = 4;
            const dim3 pg(static_cast<uint32_t>((nS + kBlock * IT - 1) / (kBlock * IT)));
            auto* cnt = static_cast<unsigned long long*>(c->count.p);
            const auto* tab = static_cast<const NPBucket*>(c->np_tab.p);
            const auto* tob = static_cast<const uint32_t*>(c->prep.p);
            with_hash(pl.hk, [&](auto h) {
                hipLaunchKernelGGL((k_pt_probe<decltype(h)::value, IT>), pg, dim3(kBlock), 0, c->ks, PS.view.keys,
                                   static_cast<uint32_t>(nS), tab, tob, ta.f, pl.seed, cnt);
            });
            PHJ_LAUNCHED(c, "k_pt_probe");
        }
        PHJ_TRY(timer_end(c));
        PHJ_TRY(mark(c, e_probe1));
        return PHJ_OK;
    }
    const size_t stride = static_cast<size_t>(P) + 1;
    PHJ_TRY(ensure(c, c->prep, stride * 3 * 4));
    PHJ_TRY(ensure(c, c->tkeys, nR * 8));
    PHJ_TRY(ensure(c, c->tpays, nR * 8));
    const size_t noffs = nR + 2 * static_cast<size_t>(P) + 1;
    PHJ_TRY(ensure(c, c->toffs, noffs * 4));
    PHJ_TRY(ensure(c, c->gcursor, noffs * 4));
    // probe schedule: small per-partition tables (the radix case) -> one wave
    // per item of <= 512 S keys; larger tables -> one workgroup per item
    const uint64_t expect_m = (nR + P - 1) / P;
    // (measured on C2: the wave schedule wins at <= ~800 S keys per partition,
    // i.e. the multi-GPU shards; the workgroup schedule at 3000)
    const uint64_t expect_s = (nS + P - 1) / P;
    const bool wave_probe = expect_m * 2 <= kProbeWaveTcap && expect_s <= 1024;
    const uint32_t kChunk = wave_probe ? 64u * kProbeWaveKPL : kBlock * 8u;
    const size_t item_bound = P + (nS + kChunk - 1) / kChunk;
    PHJ_TRY(ensure(c, c->items, item_bound * sizeof(ProbeItem)));
    PHJ_TRY(ensure(c, c->count, 32));
    PHJ_TRY(ensure(c, c->biglist, static_cast<size_t>(P) * 4));
    uint32_t* prep = static_cast<uint32_t*>(c->prep.p);
    // LDS capacities from the expected partition size (larger partitions take
    // the global-memory path; results are identical).
    const uint64_t expect = (nR + P - 1) / P;
    const uint32_t kcap = expect * 2 > 8192 ? 256u : std::max<uint32_t>(256, next_pow2_u32(static_cast<uint32_t>(expect * 2)));
    const uint32_t ocap_build = 16384;
    const uint32_t ocap_wave = std::min<uint32_t>(2048, std::max<uint32_t>(64, kcap));
    if (c->dry) return scan_u32(c, nullptr, P + 1, 3, static_cast<uint32_t>(stride));

    PHJ_TRY(mark(c, e_build0));
    PHJ_TRY(timer_begin(c, "build", nR * 32));
    hipLaunchKernelGGL(k_join_prep, dim3((P + 1 + kBlock - 1) / kBlock), dim3(kBlock), 0, c->ks, L,
                       PS.view.bounds, kChunk, prep);
    PHJ_LAUNCHED(c, "k_join_prep");
    PHJ_TRY(scan_u32(c, prep, P + 1, 3, static_cast<uint32_t>(stride)));
    const uint32_t* tkb = prep;
    const uint32_t* tob = prep + stride;
    const uint32_t* itb = prep + 2 * stride;
    hipLaunchKernelGGL(k_items_expand, dim3((P + kWaves - 1) / kWaves), dim3(kBlock), 0, c->ks, itb, tkb, tob,
                       PS.view.bounds, P, kChunk, static_cast<ProbeItem*>(c->items.p));
    PHJ_LAUNCHED(c, "k_items_expand");
    BuildArgs ba{};
    ba.L = L;
    ba.tkb = tkb;
    ba.tob = tob;
    ba.tkeys = static_cast<int64_t*>(c->tkeys.p);
    ba.tpays = static_cast<int64_t*>(c->tpays.p);
    ba.toffs = static_cast<uint32_t*>(c->toffs.p);
    ba.gcursor = static_cast<uint32_t*>(c->gcursor.p);
    ba.ocap = ocap_build;
    ba.seed = pl.seed;
    // wave-per-partition build; partitions past a wave's LDS slice go to k_build_big
    ba.biglist = static_cast<uint32_t*>(c->biglist.p);
    ba.bigcount = static_cast<uint32_t*>(c->count.p) + 2;
    PHJ_HIP(c, hipMemsetAsync(ba.bigcount, 0, 4, c->ks));
    ba.ocap = ocap_wave;
    const uint32_t sgrid = (P + kWaves - 1) / kWaves;   // one wave per partition
    const size_t slds = static_cast<size_t>(ocap_wave) * 4 * kWaves;
    with_hash(pl.hk, [&](auto h) {
        hipLaunchKernelGGL((k_build_small<decltype(h)::value, kBuildKPL>), dim3(sgrid), dim3(kBlock), slds, c->ks, ba);
    });
    PHJ_LAUNCHED(c, "k_build_small");
    ba.ocap = ocap_build;
    const size_t blds = 64 + static_cast<size_t>(ocap_build) * 4;
    with_hash(pl.hk, [&](auto h) {
        hipLaunchKernelGGL((k_build_big<decltype(h)::value>), dim3(256), dim3(kBlock), blds, c->ks, ba);
    });
    PHJ_LAUNCHED(c, "k_build_big");
    PHJ_TRY(timer_end(c));
    PHJ_TRY(mark(c, e_build1));

    PHJ_HIP(c, hipMemsetAsync(c->count.p, 0, 8, c->ks));
    ProbeArgs pa{};
    pa.skeys = PS.view.keys;
    pa.tkeys = static_cast<const int64_t*>(c->tkeys.p);
    pa.toffs = static_cast<const uint32_t*>(c->toffs.p);
    pa.items = static_cast<const ProbeItem*>(c->items.p);
    pa.nitems = itb + P;
    pa.count = static_cast<unsigned long long*>(c->count.p);
    pa.seed = pl.seed;
    PHJ_TRY(timer_begin(c, "probe", nS * 8 + nR * 8));
    // staged table slice per item: 512 keys (2 per lane) covers |R|/P up to ~300
    // (P = 65536 at 10M); larger per-partition tables stage 2048 keys or probe in place
    const bool small = expect * 2 <= 512;
    const void* kfn = with_hash(pl.hk, [&](auto h) {
        constexpr int HK = decltype(h)::value;
        return wave_probe ? reinterpret_cast<const void*>(&k_probe_wave<HK, kProbeWaveKPL, kProbeWaveTcap>)
             : small      ? reinterpret_cast<const void*>(&k_probe<HK, 8, 2>)
                          : reinterpret_cast<const void*>(&k_probe<HK, 8, 8>);
    });
    const size_t item_blocks = wave_probe ? (item_bound + kWaves - 1) / kWaves : item_bound;
    const uint32_t pgrid = chip_grid(c, item_blocks, occupancy_or(kfn, kBlock, 0, 2));
    void* kargs[] = {&pa};
    PHJ_HIP(c, hipLaunchKernel(kfn, dim3(pgrid), dim3(kBlock), kargs, 0, c->ks));
    PHJ_LAUNCHED(c, "k_probe");
    PHJ_TRY(timer_end(c));
    PHJ_TRY(mark(c, e_probe1));
    return PHJ_OK;
}

// ---- the counting join's on-chip path (phj_table.h) ----

// The build side of the on-chip join on this device's relation: pass 1 as
// hash codes, contiguous per pass-1 digit (k_hist + scan + k_scatter_codes,
// 512 x 4096 tiles), then pass 2 into final partition order (k_ht_p2, one
// workgroup per pass-1 digit). `out` receives |R| codes, `bounds` the P + 1 partition
// bounds: one build segment of build_ht (they may point into an exchange block).
// A cluster plan (pl.cluster, phj_cluster.h) stops after pass 1: `out` = the
// codes contiguous per cluster, `bounds` = the nb1 + 1 cluster bounds.
// kcol (phj_join_member): a side bound as columns is read in place, pass 1
// over its key column (8 B per tuple), whether or not a tuple copy exists.
int partition_build(phj_ctx* c, const Plan& pl, int64_t* out, uint32_t* bounds, bool kcol = false) {
    SideState& S = c->side[PHJ_SIDE_BUILD];
    c->scan_scratch = &S.partials;
    kcol = kcol && S.columns;
    if (!S.rel && !S.columns && S.n > 0) return set_err(c, PHJ_ERR_STATE, "relation not bound");
    if (!kcol && !S.rel && !c->dry && S.n > 0) return set_err(c, PHJ_ERR_STATE, "relation bound as columns: no tuple copy was packed for this pass");
    if (S.n >= (1ull << 32) - 2 * 4096) return set_err(c, PHJ_ERR_RANGE, "relation above 2^32 tuples per device");
    constexpr int BLOCK = 512, ITEMS = 8, T = BLOCK * ITEMS;
    const uint32_t n = static_cast<uint32_t>(S.n), nb = pl.nb1, P = pl.Ppad;
    const uint32_t nt = (n + T - 1) / T, hlen = nt * nb;
    PHJ_TRY(ensure(c, S.hist1, std::max<size_t>(1, hlen) * 4));
    if (!pl.cluster) PHJ_TRY(ensure(c, S.kA, std::max<size_t>(1, n) * 8));
    if (c->dry) return hlen ? scan_u32(c, nullptr, hlen, 1, hlen, c->scan_scratch) : PHJ_OK;
    if (n == 0) {
        PHJ_HIP(c, hipMemsetAsync(bounds, 0, (static_cast<size_t>(pl.cluster ? nb : P) + 1) * 4, c->ks));
        c->since_ev++;
        return PHJ_OK;
    }
    PassArgs a{};
    a.in_keys = kcol ? S.ckeys : reinterpret_cast<const int64_t*>(S.rel);
    a.out_keys = pl.cluster ? out : static_cast<int64_t*>(S.kA.p);
    a.hist = static_cast<uint32_t*>(S.hist1.p);
    a.nseg = 1;
    a.n = n;
    a.ntiles1 = nt;
    a.nbins = nb;
    a.nbits = pl.bits1;
    a.f = digit_fn(pl, 1);
    a.xcd_remap = 1;
    const uint32_t grid = (nt + 7) & ~7u;
    const size_t hlds = static_cast<size_t>(BLOCK / 64) * nb * 4;
    PHJ_TRY(timer_begin(c, "R.p1.hist", static_cast<uint64_t>(n) * (kcol ? 8 : 16)));
    with_hash(pl.hk, [&](auto h) {
        if (kcol) hipLaunchKernelGGL((k_hist<BLOCK, ITEMS, false, decltype(h)::value, true>), dim3(grid), dim3(BLOCK), hlds, c->ks, a);
        else hipLaunchKernelGGL((k_hist<BLOCK, ITEMS, true, decltype(h)::value>), dim3(grid), dim3(BLOCK), hlds, c->ks, a);
    });
    PHJ_LAUNCHED(c, "k_hist");
    PHJ_TRY(timer_end(c));
    PHJ_TRY(timer_begin(c, "R.p1.scan", static_cast<uint64_t>(hlen) * 12));
    PHJ_TRY(scan_u32(c, a.hist, hlen, 1, hlen, c->scan_scratch));   // k_ht_p2 reads d1's run from it
    PHJ_TRY(timer_end(c));
    // algorithmic bytes: the 16-B tuple (or 8-B key) read, the 8-B code written
    PHJ_TRY(timer_begin(c, "R.p1.scatter", static_cast<uint64_t>(n) * (kcol ? 16 : 24)));
    const size_t slds = scatter_codes_lds_bytes(T, nb);
    with_hash(pl.hk, [&](auto h) {
        if (kcol) hipLaunchKernelGGL((k_scatter_codes<BLOCK, ITEMS, decltype(h)::value, true>), dim3(grid), dim3(BLOCK), slds, c->ks, a);
        else hipLaunchKernelGGL((k_scatter_codes<BLOCK, ITEMS, decltype(h)::value>), dim3(grid), dim3(BLOCK), slds, c->ks, a);
    });
    PHJ_LAUNCHED(c, "k_scatter_codes");
    PHJ_TRY(timer_end(c));
    if (pl.cluster) {   // the cluster bounds from the scanned histogram
        hipLaunchKernelGGL(k_pass1_finish, dim3(1), dim3(kFinBlock), 0, c->ks, a.hist, nt, nb, n, static_cast<uint32_t>(T),
                           bounds, static_cast<uint32_t*>(nullptr));
        PHJ_LAUNCHED(c, "k_pass1_finish");
        return PHJ_OK;
    }
    HtPass2Args b{};
    b.codes = static_cast<const int64_t*>(S.kA.p);
    b.hist1 = a.hist;
    b.out = out;
    b.bounds = bounds;
    b.nt1 = nt;
    b.n = n;
    b.nb1 = nb;
    b.nb2 = pl.nb2;
    b.f2 = digit_fn(pl, 2);
    // algorithmic bytes: the codes read, written in partition order
    PHJ_TRY(timer_begin(c, "R.p2.scatter", static_cast<uint64_t>(n) * 16));
    // runs kept in registers when d1's runs average well inside kHtP2Keep
    const bool keep = static_cast<uint64_t>(n) / nb * 5 / 4 <= kHtP2Keep;
    if (keep) hipLaunchKernelGGL(k_ht_p2<true>, dim3(nb), dim3(kHtP2Block), ht_p2_lds_bytes(pl.nb2, true), c->ks, b);
    else hipLaunchKernelGGL(k_ht_p2<false>, dim3(nb), dim3(kHtP2Block), ht_p2_lds_bytes(pl.nb2, false), c->ks, b);
    PHJ_LAUNCHED(c, "k_ht_p2");
    return timer_end(c);
}

// Code tables of every final partition over `nseg` build segments (codes in
// partition order + P + 1 bounds each, e.g. the all-gathered shards), plus
// the descriptors k_probe_ht stages. nR = the codes of all segments.
int build_ht(phj_ctx* c, const Plan& pl, int nseg, const int64_t* const* codes, const uint32_t* const* bounds,
             uint64_t nR, const uint32_t* uni = nullptr) {
    if (nseg < 1 || nseg > kHtSegs) return set_err(c, PHJ_ERR_INVALID, "build segments must be in [1,16]");
    const uint32_t P = pl.Ppad;
    const uint64_t slots = 4 * nR + 2ull * P;
    if (slots >= (1ull << 32)) return set_err(c, PHJ_ERR_RANGE, "build side too large for 32-bit table slots");
    PHJ_TRY(ensure(c, c->ht_tab, slots * 8));
    PHJ_TRY(ensure(c, c->ht_desc, static_cast<size_t>(P) * 8));
    PHJ_TRY(ensure(c, c->count, 32));
    if (c->dry) return PHJ_OK;
    HtArgs a{};
    for (int g = 0; g < nseg; g++) {
        a.codes[g] = codes[g];
        a.bounds[g] = bounds[g];
    }
    a.nseg = static_cast<uint32_t>(nseg);
    a.nb1 = pl.nb1;
    a.nb2 = pl.nb2;
    a.e1 = plan_empty0(pl);
    a.table = static_cast<uint64_t*>(c->ht_tab.p);
    a.desc = static_cast<uint2*>(c->ht_desc.p);
    a.uni = uni;
    if (nseg == 1) hipLaunchKernelGGL(k_ht_fill<true>, dim3((P + kHtPpw - 1) / kHtPpw), dim3(256), 0, c->ks, a);
    else hipLaunchKernelGGL(k_ht_fill<false>, dim3((P + kHtPpw - 1) / kHtPpw), dim3(256), 0, c->ks, a);
    PHJ_LAUNCHED(c, "k_ht_fill");
    return PHJ_OK;
}

// phj_join takes the on-chip path for a 2-pass plan unless PHJ_P2PROBE=0 or a
// tuning knob changed the tile shape (the probe walks 512 x 4096 tiles).
bool use_p2probe(const phj_ctx* c, const Plan& pl, uint64_t nS, uint64_t nR) {
    (void)nS;
    return c->tune.p2probe && !pl.chained && pl.npass == 2 && tile_shape(c, pl.nb2).tile == 4096 && tile_shape(c, pl.nb2).block == 512 &&
           tile_shape(c, pl.nb1).tile == 4096 &&
           probe_ht_lds_bytes(kProbeBlock * kProbeItems, pl.nb2) <= 160 * 1024 &&
           4 * nR + 2ull * pl.Ppad < (1ull << 32) && plan_empty0(pl) != 0;
}

// phj_join takes the LDS join (phj_cluster.h) when the plan's clusters fit:
// out = the cluster plan. Needs the keys-only chunked pass 1 (512 x 4096 tiles).
// nS: the probe side (0: not known yet, e.g. the exchange geometry); it must
// take the keys-only chunked pass 1 under the cluster plan, else (a probe side
// above the pool's uint32 slot bound, ~2^32 / (kPipeRes + 1) codes per device)
// the join takes the stable pass 1 and the code tables (use_p2probe).
bool use_cluster(const phj_ctx* c, const Plan& pl, uint64_t nS, uint64_t nR, Plan& out) {
    if (!c->tune.p1_chunk || pl.stable) return false;
    if (!cluster_plan(c, pl, nR, out)) return false;
    // the chunked pass 1 runs on 512 x 4096 tiles for both of the plan's digit counts
    for (uint32_t nb : {out.nb1, out.nb2}) {
        const TileShape sh = tile_shape(c, nb);
        if (sh.tile != 4096 || sh.block != 512) return false;
    }
    if (nS > 0 && !chunked_pass1(c, out, nS, true)) return false;
    return cluster_empty0(out) != 0 && 4 * nR + 2ull * out.nb1 < (1ull << 32);
}

// The counting path a radix join of nS probe and nR build tuples takes on one
// device, and the plan that path runs: the LDS join on its cluster plan, else,
// on the plan refined by sub-partitions, the code tables or both sides fully
// partitioned. phj_join runs it, phj_prepare sizes it, phj_join_path reports
// it, phj_probe_pass1 shows its pass 1: one decision.
int radix_path(const phj_ctx* c, const Plan& asked, uint64_t nS, uint64_t nR, Plan& run) {
    if (use_cluster(c, asked, nS, nR, run)) return PHJ_PATH_LDS_JOIN;
    run = asked;
    refine_plan(c, run, nR);
    return use_p2probe(c, run, nS, nR) ? PHJ_PATH_CODE_TABLES : PHJ_PATH_PARTITIONED;
}

// Probe a probe-side pass-1 output (partition_state p1_only) against the
// tables of build_ht; the count lands in (clear) or is added to c->count.
int probe_ht(phj_ctx* c, const Plan& pl, SideState& PS, bool clear = true) {
    if (clear) PHJ_HIP(c, hipMemsetAsync(c->count.p, 0, 16, c->ks));
    if (PS.nt2 == 0) return PHJ_OK;
    HtProbeArgs pa{};
    pa.a = PS.p2;
    pa.desc = static_cast<const uint2*>(c->ht_desc.p);
    pa.table = static_cast<const uint64_t*>(c->ht_tab.p);
    pa.count = static_cast<unsigned long long*>(c->count.p);
    if (PS.chunk_check) {   // its error word is folded into the count pair
        pa.err = static_cast<const uint32_t*>(PS.ccur.p) + chunk_err_word(PS.plan.nb1);
        PS.chunk_check = false;
    }
    pa.seed = pl.seed;
    pa.e1 = plan_empty0(pl);
    pa.nb2 = pl.nb2;
    constexpr int B = kProbeBlock, I = kProbeItems;
    const size_t lds = probe_ht_lds_bytes(B * I, pl.nb2);
    // a keys-only pass 1 wrote codes (k_chunk_codes); a stable pass 1 left whole tuples
    // (the chunked pass-1 output is always codes; a radix plan's d2 is a bit field)
    const bool radix = pl.mode == 0 && pl.sub_bits == 0;
    const void* kfn = PS.hcoded ? (radix ? reinterpret_cast<const void*>(&k_probe_ht<B, I, kHashed, kProbeRadix | kProbeChunked>)
                                         : reinterpret_cast<const void*>(&k_probe_ht<B, I, kHashed, kProbeChunked>))
                      : with_hash(pl.hk, [](auto h) {
                            return reinterpret_cast<const void*>(&k_probe_ht<B, I, decltype(h)::value>);
                        });
    // persistent: as many workgroups as fit the chip at once (a multiple of 8:
    // XCD x owns tiles [x, x + 1) * ntiles / 8), never many more than tiles
    const int per_cu = std::min<int>(occupancy_or(kfn, B, lds, 2), static_cast<int>(160 * 1024 / lds));
    const uint32_t want = (PS.nt2 + 7) & ~7u;
    const uint32_t grid = std::max<uint32_t>(8, std::min<uint32_t>(want, static_cast<uint32_t>(per_cu) * c->num_cus) & ~7u);
    void* kargs[] = {&pa};
    PHJ_HIP(c, hipLaunchKernel(kfn, dim3(grid), dim3(B), kargs, lds, c->ks));
    PHJ_LAUNCHED(c, "k_probe_ht");
    return PHJ_OK;
}

// A stale chunk table met by a chunked pass (phj_partition.h chunk_err_word):
// the pass wrote nothing through it, and the join reports PHJ_ERR_STATE. Both
// sides' tables are cleared before their next pass.
int chunk_table_error(phj_ctx* c, uint32_t bits) {
    for (SideState& S : c->side) {
        S.ctab_dirty = true;
        S.chunk_check = false;
    }
    return set_err(c, PHJ_ERR_STATE, "chunked pass 1 read a chunk-table entry out of range (stale table, error bits " +
                                         std::to_string(bits) + "); nothing was written through it");
}

// The error words of chunked passes not folded into a count (a 4-B read back
// per side; the default on-chip join folds S's into the count instead).
int check_chunk_errors(phj_ctx* c) {
    for (SideState& S : c->side) {
        if (!S.chunk_check) continue;
        S.chunk_check = false;
        uint32_t e = 0;
        PHJ_HIP(c, hipMemcpyAsync(&e, static_cast<const uint32_t*>(S.ccur.p) + chunk_err_word(S.plan.nb1), 4,
                                  hipMemcpyDeviceToHost, c->ks));
        PHJ_HIP(c, hipStreamSynchronize(c->ks));
        if (e) return chunk_table_error(c, e);
    }
    return PHJ_OK;
}

// The LDS join over a cluster plan: the HBM tables of the clusters beyond the
// LDS limit (k_cluster_big_fill, on the current launch stream: R's chain),
// then (probe_cluster, on the main stream) k_cluster_probe over the probe
// side's pass-1 tiles. `nseg` build segments of codes contiguous per cluster
// and nb1 + 1 bounds each; nR = their codes. The count pair is added to.
// RT (tile mode, one device): R's chunked code pass; its tiles are the runs,
// its cluster offsets (bounds1) give each cluster's size and first code.
ClusterArgs cluster_args(phj_ctx* c, const Plan& pl, int nseg, const int64_t* const* codes,
                         const uint32_t* const* bounds, SideState* RT = nullptr) {
    ClusterArgs a{};
    if (RT) {
        nseg = 1;
        a.r_codes[0] = RT->p2.in_keys;
        a.r_bounds[0] = static_cast<const uint32_t*>(RT->bounds1.p);
        a.rt_base = RT->p2.tile_base;
        a.rt_start = RT->p2.tile_start;
        a.rt_cnt = RT->p2.tile_cnt;
        a.r_pool = RT->p2.in_keys;
    } else {
        for (int g = 0; g < nseg; g++) {
            a.r_codes[g] = codes[g];
            a.r_bounds[g] = bounds[g];
        }
    }
    a.nseg = static_cast<uint32_t>(nseg);
    a.nb1 = pl.nb1;
    a.cap = static_cast<uint32_t>(c->tune.cl_cap);
    a.lim = cl_lim(a.cap);
    a.e1 = cluster_empty0(pl);
    a.gtab = static_cast<uint64_t*>(c->ht_tab.p);
    a.count = static_cast<unsigned long long*>(c->count.p);
    return a;
}

int cluster_big_fill(phj_ctx* c, const Plan& pl, int nseg, const int64_t* const* codes, const uint32_t* const* bounds,
                     uint64_t nR, SideState* RT = nullptr) {
    if (nseg < 1 || nseg > kHtSegs) return set_err(c, PHJ_ERR_INVALID, "build segments must be in [1,16]");
    const uint64_t slots = 4 * nR + 2ull * pl.nb1;
    if (slots >= (1ull << 32)) return set_err(c, PHJ_ERR_RANGE, "build side too large for 32-bit table slots");
    PHJ_TRY(ensure(c, c->ht_tab, slots * 8));
    PHJ_TRY(ensure(c, c->count, 32));
    if (c->dry) return PHJ_OK;
    ClusterArgs a = cluster_args(c, pl, nseg, codes, bounds, RT);
    hipLaunchKernelGGL(k_cluster_big_fill, dim3(pl.nb1), dim3(256), 0, c->ks, a);
    PHJ_LAUNCHED(c, "k_cluster_big_fill");
    return PHJ_OK;
}

// The pinned count word pair (count_pin) and its device side; false: the
// count comes back by a copy (get_count).
bool count_pin_ready(phj_ctx* c) {
    if (c->count_pin) return true;
    if (c->count_pin_failed) return false;
    void* h = nullptr;
    void* d = nullptr;
    if (hipHostMalloc(&h, 64, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
        hipHostGetDevicePointer(&d, h, 0) != hipSuccess || ensure(c, c->cl_done, 4) != PHJ_OK ||
        hipMemset(c->cl_done.p, 0, 4) != hipSuccess) {
        (void)hipGetLastError();
        if (h) (void)hipHostFree(h);
        c->count_pin_failed = true;
        return false;
    }
    c->count_pin = static_cast<unsigned long long*>(h);
    c->count_pin_dev = static_cast<unsigned long long*>(d);
    return true;
}

// pin: the last kernel also writes the count pair to count_pin (get_count
// then only synchronises; one device-to-host copy fewer per join)
int probe_cluster(phj_ctx* c, const Plan& pl, SideState& PS, int nseg, const int64_t* const* codes,
                  const uint32_t* const* bounds, SideState* RT = nullptr, bool pin = false) {
    if (c->dry || PS.nt2 == 0) return PHJ_OK;
    if (!PS.hcoded) return set_err(c, PHJ_ERR_STATE, "the LDS join needs the keys-only pass 1 (codes)");
    ClusterArgs a = cluster_args(c, pl, nseg, codes, bounds, RT);
    SideState& RS = c->side[PHJ_SIDE_BUILD];
    if (RS.chunk_check) {   // R's chunked pass-1 error word, folded into the count pair as S's
        a.err_r = static_cast<const uint32_t*>(RS.ccur.p) + chunk_err_word(RS.plan.nb1);
        RS.chunk_check = false;
    }
    a.s_codes = PS.p2.in_keys;
    a.tile_base = PS.p2.tile_base;
    a.tile_seg = PS.p2.tile_seg;
    a.tile_start = PS.p2.tile_start;
    a.tile_cnt = PS.p2.tile_cnt;
    if (PS.chunk_check) {   // its error word is folded into the count pair
        a.err = static_cast<const uint32_t*>(PS.ccur.p) + chunk_err_word(PS.plan.nb1);
        PS.chunk_check = false;
    }
    // the clock split: words 2-3 of the count buffer, cleared with the count
    // pair by the pass-1 bookkeeping kernel (no memset per join)
    if (c->tune.timers) {
        a.split = static_cast<unsigned long long*>(c->count.p) + 2;
        c->split_words = a.split;
    }
    constexpr int B = kClBlock, I = kClItems;
    const size_t lds = cluster_lds_bytes(a.cap);   // the table + its 16-bit bucket fill counters
    constexpr bool PR = PHJ_CL_PROF != 0;   // measurement build: the builds' section clocks
    if (PR) {
        PHJ_TRY(ensure(c, c->cl_prof, 64 * 8));
        a.prof = static_cast<unsigned long long*>(c->cl_prof.p);
        PHJ_HIP(c, hipMemsetAsync(a.prof, 0, kClProfWords * 8, c->ks));
    }
    // three tiles of codes in flight, the next cluster's R codes prefetched
    // (measured: one / two tiles 0.406 / 0.360 ms against 0.355 at C2; tables by
    // 64-bit compare-and-swap 0.082 ms of builds against 0.055 by fill counters)
    // with the hot table of S's pass 1 (hot_begin), the join resolves its
    // weights: the entries R holds add theirs to the count (an empty R holds none)
    if (c->hot_on && RT && &PS == &c->side[PHJ_SIDE_PROBE]) {
        const uint32_t* st = static_cast<const uint32_t*>(c->hot.p);
        a.hot_code = reinterpret_cast<const unsigned long long*>(st + kHotCounters);
        a.hot_w = a.hot_code + static_cast<size_t>(pl.nb1) * kHotPer;
        a.hot_ctl = reinterpret_cast<const uint32_t*>(a.hot_w + static_cast<size_t>(pl.nb1) * kHotPer);
        a.hot_min_mass = c->hot_min_mass;
    }
    const void* kfn = !RT          ? reinterpret_cast<const void*>(&k_cluster_probe<B, I, 3, true, PR, false>)
                      : a.hot_code ? reinterpret_cast<const void*>(&k_cluster_probe<B, I, 3, true, PR, true, true>)
                                   : reinterpret_cast<const void*>(&k_cluster_probe<B, I, 3, true, PR, true>);
    const int per_cu = std::max(1, std::min<int>(occupancy_or(kfn, B, lds, 1), static_cast<int>(160 * 1024 / (lds + 256))));
    // persistent, a multiple of 8 (XCD-grouped ranges), never many more than tiles
    const uint32_t want = (PS.nt2 + 7) & ~7u;
    const uint32_t grid = std::max<uint32_t>(8, std::min<uint32_t>(want, static_cast<uint32_t>(per_cu) * c->num_cus) & ~7u);
    void* kargs[] = {&a};
    PHJ_TRY(launch_kernel(c, kfn, dim3(grid), dim3(B), kargs, lds, "k_cluster_probe"));
    if (PR) {   // diagnostics (measurement build): synchronous, to stderr, in microseconds summed over workgroups
        unsigned long long h[kClProfWords] = {};
        PHJ_HIP(c, hipMemcpyAsync(h, a.prof, sizeof(h), hipMemcpyDeviceToHost, c->ks));
        PHJ_HIP(c, hipStreamSynchronize(c->ks));
        std::fprintf(stderr, "cl_prof grid %u: cold %.1f us, clear+runs %.1f us, inserts %.1f us, prefetch %.1f us; builds %llu, cold %llu\n",
                     grid, h[0] / 100.0, h[1] / 100.0, h[2] / 100.0, h[3] / 100.0, h[4], h[5]);
    }
    // the big clusters' tiles against their HBM tables (workgroups of the
    // other clusters return at once)
    a.split = nullptr;
    a.err = nullptr;
    a.err_r = nullptr;
    if (pin && c->tune.count_pin && count_pin_ready(c)) {
        // a value no launch writes (failed holds error bits): get_count falls
        // back to the copy if the kernel left it
        reinterpret_cast<volatile unsigned long long*>(c->count_pin)[1] = ~0ull;
        a.host_out = c->count_pin_dev;
        a.done = static_cast<uint32_t*>(c->cl_done.p);
        c->count_pinned = true;
        // S's chunk state is read no more after this launch: cleared for the next join
        a.s_clear = static_cast<uint4*>(PS.ccur.p);
        a.s_clear16 = static_cast<uint32_t>(chunk_state_bytes(PS.plan.nb1) / 16);
        c->s_zero_pending = PS.ccur.p;
        c->s_zero_pending_bytes = chunk_state_bytes(PS.plan.nb1);
    }
    hipLaunchKernelGGL(k_cluster_probe_big, dim3(std::max<uint32_t>(kProbeBigGrid, (pl.nb1 + 255) / 256)), dim3(256), 0, c->ks, a);
    PHJ_LAUNCHED(c, "k_cluster_probe_big");
    return PHJ_OK;
}

// The count comes back through a pinned host word (a pageable destination is
// staged by the runtime: a slower copy on the step's critical path). pair:
// the on-chip probes' {count, failed}, failed set when S's pass 1 met a stale
// chunk table (fold_pass1_error).
int get_count(phj_ctx* c, uint64_t* out, bool pair = false) {
    if (c->count_pinned) {   // written by the join's last workgroup (probe_cluster)
        c->count_pinned = false;
        const volatile unsigned long long* v = c->count_pin;
        if (c->defer_timers) {
            // no event is read in this join: poll the pinned word (the
            // driver's stream synchronisation wakes later), asking every
            // 4096 polls whether the stream has finished without it
            for (uint32_t i = 1; v[1] == ~0ull; i++) {
                if ((i & 4095u) == 0) {
                    const hipError_t q = hipStreamQuery(c->ks);
                    if (q == hipSuccess) break;
                    if (q != hipErrorNotReady) PHJ_HIP(c, q);
                }
                __builtin_ia32_pause();
            }
            std::atomic_thread_fence(std::memory_order_acquire);
        } else {
            PHJ_HIP(c, hipStreamSynchronize(c->ks));
        }
        const unsigned long long failed = v[1];
        if (failed == 0) {   // the last workgroup cleared S's chunk state
            c->s_zeroed = c->s_zero_pending;
            c->s_zeroed_bytes = c->s_zero_pending_bytes;
        }
        c->s_zero_pending = nullptr;
        if (failed != ~0ull) {
            *out = v[0];
            if (pair && failed) {
                c->side[PHJ_SIDE_PROBE].chunk_check = true;   // read its word for the message
                const int rc = check_chunk_errors(c);
                return rc != PHJ_OK ? rc : chunk_table_error(c, 0);
            }
            return check_chunk_errors(c);
        }
    }
    if (!c->count_host && hipHostMalloc(reinterpret_cast<void**>(&c->count_host), 16, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        c->count_host = nullptr;
    }
    unsigned long long h[2] = {0, 0};
    unsigned long long* dst = c->count_host ? c->count_host : h;
    PHJ_HIP(c, hipMemcpyAsync(dst, c->count.p, pair ? 16 : 8, hipMemcpyDeviceToHost, c->ks));
    PHJ_HIP(c, hipStreamSynchronize(c->ks));
    *out = dst[0];
    if (pair && dst[1]) {
        c->side[PHJ_SIDE_PROBE].chunk_check = true;   // read its word for the message
        const int rc = check_chunk_errors(c);
        return rc != PHJ_OK ? rc : chunk_table_error(c, 0);
    }
    return check_chunk_errors(c);
}

// R partitioned by the radix bits b0 + b1 of its hash codes under p's hash and
// seed, whatever else p asks for: the plan of a table build's regions.
int radix_plan(phj_ctx* c, const phj_join_params* p, uint32_t b0, uint32_t b1, Plan& pl) {
    phj_join_params pp = *p;
    pp.algo = PHJ_ALGO_RADIX;
    pp.num_partitions = 0;
    pp.flags = 0;
    pp.radix_bits[0] = static_cast<uint8_t>(b0);
    pp.radix_bits[1] = static_cast<uint8_t>(b1);
    return make_plan(c, &pp, pl);
}

// ... into the 2^rbits regions of a bucket table (np_build, index_build): one
// pass up to 8 bits, beyond two balanced ones.
int region_plan(phj_ctx* c, const phj_join_params* p, uint32_t rbits, Plan& pl) {
    const uint32_t b1 = rbits <= 8 ? 0 : rbits / 2;
    return radix_plan(c, p, rbits - b1, b1, pl);
}

// The closing of every NoPartitioning form: no partition phase, build = [e0, e1), probe = [e1, e2).
int np_times(phj_ctx* c, hipEvent_t e0, hipEvent_t e1, hipEvent_t e2, phj_join_result* r) {
    r->partition_ms = 0;
    r->build_ms = elapsed(c, e0, e1);
    r->probe_ms = elapsed(c, e1, e2);
    r->total_ms = elapsed(c, e0, e2);
    r->num_partitions = 0;
    return fill_timers(c, r);
}

// Region code tables (phj_table.h) over the build side, as the NoPartitioning
// count and phj_join_member probe them: R partitioned into 2^k regions of ~300
// codes by two radix passes of its hash codes, one code table per region.
// marks: a buffer sized to one byte per table slot after the workspace, before
// the first event (phj_join_member's slot marks), or null.
// kcol: partition_build's (a side bound as columns is read from its key column).
// *e0 is recorded before the first kernel. Under phj_prepare (c->dry) only the
// workspace is sized.
struct CtBuild {
    Plan pl;
    uint32_t P = 0;             // regions
    uint64_t slot_bound = 0;    // table slots
    const int64_t* rcodes = nullptr;
    const uint32_t* rbnd = nullptr;
    uint32_t* uni = nullptr;
    hipEvent_t e0 = nullptr;
};

int ct_build(phj_ctx* c, const phj_join_params* p, bool kcol, DevBuf* marks, CtBuild& t) {
    const SideState& R = c->side[PHJ_SIDE_BUILD];
    uint32_t k = 2;
    while (k < 22 && (R.n >> k) > 300) k++;
    PHJ_TRY(radix_plan(c, p, k - k / 2, k / 2, t.pl));
    t.P = t.pl.Ppad;
    t.slot_bound = 4 * R.n + 2ull * t.P;
    PHJ_TRY(ensure(c, c->r_codes, std::max<uint64_t>(1, R.n) * 8));
    PHJ_TRY(ensure(c, c->r_bounds, (static_cast<size_t>(t.P) + 1) * 4));
    PHJ_TRY(ensure(c, c->np_uni, 16));
    PHJ_TRY(ensure(c, c->count, 32));
    if (marks) PHJ_TRY(ensure(c, *marks, t.slot_bound));
    t.rcodes = static_cast<const int64_t*>(c->r_codes.p);
    t.rbnd = static_cast<const uint32_t*>(c->r_bounds.p);
    t.uni = static_cast<uint32_t*>(c->np_uni.p);
    if (c->dry) {
        PHJ_TRY(partition_build(c, t.pl, static_cast<int64_t*>(c->r_codes.p), static_cast<uint32_t*>(c->r_bounds.p), kcol));
        return build_ht(c, t.pl, 1, &t.rcodes, &t.rbnd, R.n, t.uni);
    }
    PHJ_TRY(mark(c, &t.e0));
    // the partition is part of the build (its R.* timers show it)
    PHJ_TRY(partition_build(c, t.pl, static_cast<int64_t*>(c->r_codes.p), static_cast<uint32_t*>(c->r_bounds.p), kcol));
    // algorithmic bytes: the codes read, the tables written (~1.7 slots per code)
    PHJ_TRY(timer_begin(c, "np.build", R.n * 8 * 3));
    hipLaunchKernelGGL(k_np_ct_plan, dim3(1), dim3(256), 0, c->ks, t.rbnd, t.P, t.slot_bound, t.uni);
    PHJ_LAUNCHED(c, "k_np_ct_plan");
    PHJ_TRY(build_ht(c, t.pl, 1, &t.rcodes, &t.rbnd, R.n, t.uni));
    return timer_end(c);
}

// The NoPartitioning count over region code tables (k_np_probe_ct): ct_build
// (the build), then S probed unpartitioned.
int join_nopart_ct(phj_ctx* c, const phj_join_params* p, phj_join_result* r) {
    SideState& R = c->side[PHJ_SIDE_BUILD];
    SideState& S = c->side[PHJ_SIDE_PROBE];
    CtBuild t;
    PHJ_TRY(ct_build(c, p, false, nullptr, t));
    if (c->dry) return PHJ_OK;
    const Plan& pl = t.pl;
    const uint32_t P = t.P;
    auto* uni = t.uni;
    hipEvent_t e1, e2;
    PHJ_TRY(mark(c, &e1));
    PHJ_HIP(c, hipMemsetAsync(c->count.p, 0, 8, c->ks));
    if (S.n > 0) {
        // algorithmic bytes: S's tuples read once (16 B), R's tables (~2 slots per code) once
        PHJ_TRY(timer_begin(c, "np.probe", S.n * 16 + R.n * 16));
        constexpr int IT = 4;
        const void* kfn = with_hash(p->hash, [](auto h) {
            return reinterpret_cast<const void*>(&k_np_probe_ct<decltype(h)::value, IT>);
        });
        const uint32_t grid = chip_grid(c, (S.n + 256ull * IT - 1) / (256ull * IT), occupancy_or(kfn, 256, 0, 8));
        const auto* S_rel = reinterpret_cast<const longlong2*>(S.rel);
        const auto* tab = static_cast<const uint64_t*>(c->ht_tab.p);
        const auto* dsc = static_cast<const uint2*>(c->ht_desc.p);
        const uint32_t* un = uni;
        auto* cnt = static_cast<unsigned long long*>(c->count.p);
        uint64_t nS64 = S.n, seed = p->hash_seed, e1 = plan_empty0(pl);
        uint32_t Pv = P;
        void* kargs[] = {const_cast<longlong2**>(&S_rel), &nS64, const_cast<uint64_t**>(&tab), const_cast<uint2**>(&dsc),
                         const_cast<uint32_t**>(&un), &Pv, &seed, &e1, &cnt};
        PHJ_HIP(c, hipLaunchKernel(kfn, dim3(grid), dim3(256), kargs, 0, c->ks));
        PHJ_LAUNCHED(c, "k_np_probe_ct");
        PHJ_TRY(timer_end(c));
    }
    PHJ_TRY(mark(c, &e2));
    uint64_t m = 0;
    PHJ_TRY(get_count(c, &m));
    r->matches = m;
    r->algorithmic_bytes = R.n * (16 + 8 + 8 + 8) + R.n * 24 + S.n * 16 + R.n * 16;
    return np_times(c, t.e0, e1, e2, r);
}

// phj_join_member (phj_member.h): the build half of join_nopart_ct over keys
// alone, then the membership probe (mask, count and, with the build side
// asked, slot marks) and the pass over R that reads the marks.
int join_member(phj_ctx* c, const phj_join_params* p, uint32_t sides, uint8_t* probe_mask, uint8_t* build_mask,
                phj_join_result* r, phj_member_counts* n) {
    const char* what = "phj_join_member";
    if (!c || !r || !n) return PHJ_ERR_INVALID;
    if (c->group) return set_err(c, PHJ_ERR_STATE, std::string(what) + ": single-device contexts only");
    if (!p) return set_err(c, PHJ_ERR_INVALID, "null params");
    if (sides == 0 || (sides & ~static_cast<uint32_t>(PHJ_MEMBER_PROBE | PHJ_MEMBER_BUILD)))
        return set_err(c, PHJ_ERR_INVALID, std::string(what) + ": sides must be a set of PHJ_MEMBER_PROBE / PHJ_MEMBER_BUILD");
    if (p->algo != PHJ_ALGO_NO_PARTITIONING && p->algo != PHJ_ALGO_RADIX)
        return set_err(c, PHJ_ERR_INVALID, "Unrecognized join algorithm");
    if (p->hash != PHJ_HASH_XXH3 && p->hash != PHJ_HASH_MURMUR3) return set_err(c, PHJ_ERR_INVALID, "unknown hash function");
    if (p->algo == PHJ_ALGO_RADIX) {   // the usual validation; the plan itself is not used
        Plan asked;
        PHJ_TRY(make_plan(c, p, asked));
    }
    SideState& R = c->side[PHJ_SIDE_BUILD];
    SideState& S = c->side[PHJ_SIDE_PROBE];
    const bool want_s = (sides & PHJ_MEMBER_PROBE) != 0, want_b = (sides & PHJ_MEMBER_BUILD) != 0;
    if ((want_s && !probe_mask && S.n > 0) || (want_b && !build_mask && R.n > 0))
        return set_err(c, PHJ_ERR_INVALID, std::string(what) + ": a side that is asked needs its mask");
    for (const SideState* X : {&R, &S})
        if (!X->rel && !X->columns && X->n > 0) return set_err(c, PHJ_ERR_STATE, "relation not bound");
    if (R.n >= (1ull << 30)) return set_err(c, PHJ_ERR_RANGE, std::string(what) + ": build side of 2^30 rows or more");
    PHJ_TRY(begin_call(c));
    std::memset(r, 0, sizeof(*r));
    std::memset(n, 0, sizeof(*n));
    // an empty side joins to nothing: the other side's mask is all 0, no join runs
    if (R.n == 0 || S.n == 0) {
        if (want_s && S.n > 0) PHJ_HIP(c, hipMemsetAsync(probe_mask, 0, S.n, c->ks));
        if (want_b && R.n > 0) PHJ_HIP(c, hipMemsetAsync(build_mask, 0, R.n, c->ks));
        PHJ_HIP(c, hipStreamSynchronize(c->ks));
        return PHJ_OK;
    }
    // keys alone: a side bound as columns is read from its key column, packed or not
    const bool r_keys = R.columns, s_keys = S.columns;
    const uint64_t rk = r_keys ? 8 : 16, sk = s_keys ? 8 : 16;
    CtBuild t;
    PHJ_TRY(ct_build(c, p, r_keys, want_b ? &c->member_marks : nullptr, t));   // (marks: one byte per table slot)
    const Plan& pl = t.pl;
    const uint32_t P = t.P;
    const uint64_t slot_bound = t.slot_bound;
    auto* uni = t.uni;
    auto* cnt = static_cast<unsigned long long*>(c->count.p);
    hipEvent_t e1, e2;
    PHJ_TRY(mark(c, &e1));
    PHJ_HIP(c, hipMemsetAsync(cnt, 0, 32, c->ks));
    const uint64_t per = 256ull * kMemberItems;
    {
        // algorithmic bytes: S's keys read once, R's tables (~2 slots per code) once, the mask
        // written; with marks the slot bytes cleared and (at most) one stored per hit's line
        PHJ_TRY(timer_begin(c, "member.probe", S.n * sk + R.n * 16 + (want_s ? S.n : 0) + (want_b ? slot_bound : 0)));
        if (want_b) PHJ_HIP(c, hipMemsetAsync(c->member_marks.p, 0, slot_bound, c->ks));
        const void* kfn = with_hash(p->hash, [&](auto h) {
            constexpr int HK = decltype(h)::value;
            auto pick = [&](auto KEYS, auto MARK) {
                constexpr bool K = decltype(KEYS)::value, M = decltype(MARK)::value;
                return reinterpret_cast<const void*>(&k_np_member_probe<HK, kMemberItems, K, M>);
            };
            return s_keys ? (want_b ? pick(std::true_type{}, std::true_type{}) : pick(std::true_type{}, std::false_type{}))
                          : (want_b ? pick(std::false_type{}, std::true_type{}) : pick(std::false_type{}, std::false_type{}));
        });
        const uint32_t grid = chip_grid(c, (S.n + per - 1) / per, occupancy_or(kfn, 256, 0, 8));
        MemberProbeArgs a{};
        a.keys = s_keys ? S.ckeys : reinterpret_cast<const int64_t*>(S.rel);
        a.n = S.n;
        a.table = static_cast<const uint64_t*>(c->ht_tab.p);
        a.desc = static_cast<const uint2*>(c->ht_desc.p);
        a.uni = uni;
        a.P = P;
        a.seed = p->hash_seed;
        a.e1 = plan_empty0(pl);
        a.mask = want_s ? probe_mask : nullptr;
        a.marks = want_b ? static_cast<uint8_t*>(c->member_marks.p) : nullptr;
        a.count = cnt;
        void* kargs[] = {&a};
        PHJ_TRY(launch_kernel(c, kfn, dim3(grid), dim3(256), kargs, 0, "k_np_member_probe"));
        PHJ_TRY(timer_end(c));
    }
    if (want_b) {
        // algorithmic bytes: R's keys read again, a bucket and a mark per row, the mask written
        PHJ_TRY(timer_begin(c, "member.build", R.n * (rk + 16 + 1 + 1)));
        const void* kfn = with_hash(p->hash, [&](auto h) {
            constexpr int HK = decltype(h)::value;
            return r_keys ? reinterpret_cast<const void*>(&k_member_build<HK, true>)
                          : reinterpret_cast<const void*>(&k_member_build<HK, false>);
        });
        const uint32_t grid = chip_grid(c, (R.n + per - 1) / per, 8);
        MemberBuildArgs a{};
        a.keys = r_keys ? R.ckeys : reinterpret_cast<const int64_t*>(R.rel);
        a.n = R.n;
        a.table = static_cast<const uint64_t*>(c->ht_tab.p);
        a.desc = static_cast<const uint2*>(c->ht_desc.p);
        a.uni = uni;
        a.P = P;
        a.seed = p->hash_seed;
        a.e1 = plan_empty0(pl);
        a.mask = build_mask;
        a.marks = static_cast<const uint8_t*>(c->member_marks.p);
        a.count = cnt + 1;
        void* kargs[] = {&a};
        PHJ_TRY(launch_kernel(c, kfn, dim3(grid), dim3(256), kargs, 0, "k_member_build"));
        PHJ_TRY(timer_end(c));
    }
    PHJ_TRY(mark(c, &e2));
    unsigned long long h[3] = {0, 0, 0};   // {probe rows matched, build rows matched, a build key was not found}
    PHJ_HIP(c, hipMemcpyAsync(h, cnt, sizeof(h), hipMemcpyDeviceToHost, c->ks));
    PHJ_HIP(c, hipStreamSynchronize(c->ks));
    if (h[2]) return set_err(c, PHJ_ERR_STATE, std::string(what) + ": a build key was not found in its region's table");
    n->probe_matched = h[0];
    n->build_matched = want_b ? h[1] : 0;
    r->matches = h[0];
    r->algorithmic_bytes = R.n * (rk + (rk + 8) + 16) + R.n * 24 + S.n * sk + R.n * 16 + (want_s ? S.n : 0) +
                           (want_b ? slot_bound + R.n * (rk + 16 + 1 + 1) : 0);
    return np_times(c, t.e0, e1, e2, r);
}

// The geometry of a bucket table built by regions (np_build, index_build):
// `rows` keys at table_ratio (0: the default) slots each in buckets of `slots`,
// in 2^rbits regions of <= region_buckets buckets (LDS-sized; nbr_max: the most
// the last doubling may leave a region). what: the prefix of the range message.
int table_geometry(phj_ctx* c, uint64_t rows, double table_ratio, uint32_t slots, uint32_t region_buckets, uint32_t nbr_max,
                   const char* what, NPHome& g) {
    const double ratio = table_ratio > 0 ? table_ratio : kNPDefaultRatio;
    if (ratio < 1.0) return set_err(c, PHJ_ERR_INVALID, "table_ratio must be >= 1");
    const double nbd = std::ceil(static_cast<double>(rows) * ratio / slots);
    if (nbd >= 4294967295.0) return set_err(c, PHJ_ERR_RANGE, std::string(what) + "table too large");
    const uint32_t nb0 = std::max<uint32_t>(1, static_cast<uint32_t>(nbd));
    g = NPHome{nb0, nb0, 0, 0};
    g.rbits = std::min<uint32_t>(22, std::max<uint32_t>(1, ceil_log2((nb0 + region_buckets - 1) / region_buckets)));
    g.nbr = (nb0 + (1u << g.rbits) - 1) >> g.rbits;
    const uint64_t nbw = static_cast<uint64_t>(g.nbr) << g.rbits;
    if (nbw >= 4294967295ull || g.nbr > nbr_max) return set_err(c, PHJ_ERR_RANGE, std::string(what) + "table too large");
    g.nb = static_cast<uint32_t>(nbw);
    return PHJ_OK;
}

// The NoPartitioning bucket table (np_tab, np_pays) over the build side: R
// radix-partitioned into the table's regions, one workgroup per region, then
// the overflow list. g: the table's geometry. slots32: every slot index
// b * 7 + s must stay below kNoMatch (the materialising probes store it in 32
// bits). *e0 is recorded before the first kernel. Under phj_prepare (c->dry)
// only the workspace is sized.
// pay: what np_pays holds (PaySrc::RowNumber: each build tuple's row number).
int np_build(phj_ctx* c, const phj_join_params* p, bool slots32, NPHome& g, hipEvent_t* e0, PaySrc pay = PaySrc::Bound) {
    SideState& R = c->side[PHJ_SIDE_BUILD];
    PHJ_TRY(table_geometry(c, R.n, p->table_ratio, kNPSlots, kNPRegionBuckets, 2 * kNPRegionBuckets, "", g));
    const uint32_t nb = g.nb;
    // the materialising probe stores a match as the uint32 slot b * 7 + s, and
    // kNoMatch (0xffffffff) must stay out of that range
    if (slots32 && static_cast<uint64_t>(nb) * kNPSlots >= kNoMatch)
        return set_err(c, PHJ_ERR_RANGE, "materialised NoPartitioning join: table above 2^32 - 1 slots");
    PHJ_TRY(ensure(c, c->np_tab, static_cast<size_t>(nb) * sizeof(NPBucket)));
    PHJ_TRY(ensure(c, c->np_pays, static_cast<size_t>(nb) * kNPSlots * 8));
    PHJ_TRY(ensure(c, c->count, 8));
    PHJ_TRY(ensure(c, c->np_ovf, R.n * 16));
    PHJ_TRY(ensure(c, c->np_ovfb, R.n * 4));
    PHJ_TRY(ensure(c, c->np_ovfn, 4));
    Plan rp;
    PHJ_TRY(region_plan(c, p, g.rbits, rp));
    if (c->dry) return partition_side(c, PHJ_SIDE_BUILD, rp, false, nullptr, pay);
    const uint32_t nR = static_cast<uint32_t>(R.n);
    PHJ_TRY(mark(c, e0));
    {
        // the partition is part of the build (its R.* timers show it)
        PHJ_TRY(partition_side(c, PHJ_SIDE_BUILD, rp, false, nullptr, pay));
        const phj_partitioned& v = R.view;
        PHJ_TRY(timer_begin(c, "np.build", static_cast<uint64_t>(nR) * 32 + static_cast<uint64_t>(nb) * 64));
        PHJ_HIP(c, hipMemsetAsync(c->np_ovfn.p, 0, 4, c->ks));
        const size_t lds = static_cast<size_t>(g.nbr) * (kNPSlots * 8 + 4);
        auto* ovn = static_cast<uint32_t*>(c->np_ovfn.p);
        auto* ov = static_cast<longlong2*>(c->np_ovf.p);
        auto* ovb = static_cast<uint32_t*>(c->np_ovfb.p);
        auto* tab = static_cast<NPBucket*>(c->np_tab.p);
        auto* pays = static_cast<int64_t*>(c->np_pays.p);
        const dim3 grid(1u << g.rbits);
        with_hash(p->hash, [&](auto h) {
            hipLaunchKernelGGL((k_np_build_region<decltype(h)::value>), grid, dim3(kBlock), lds, c->ks, v.keys,
                               v.payloads, v.bounds, g, tab, pays, p->hash_seed, ovn, ov, ovb);
        });
        PHJ_LAUNCHED(c, "k_np_build_region");
        hipLaunchKernelGGL(k_np_build_overflow, dim3(64), dim3(kBlock), 0, c->ks, ovn, ov, ovb, tab, pays, nb);
        PHJ_LAUNCHED(c, "k_np_build_overflow");
        PHJ_TRY(timer_end(c));
    }
    return PHJ_OK;
}

// The NoPartitioning form of the row and aggregate joins (one probe of the
// bucket table over the bound S, four tuples per thread): what comes before
// the first probe kernel (np_setup) and at the end (np_times), as FusedJoin
// has it for the radix form. The drivers see either one as a JoinForm.
struct NPJoin {
    NPHome g{};
    hipEvent_t e0 = nullptr, e1 = nullptr;   // around the build
    uint32_t grid = 0;
    const longlong2* S_rel = nullptr;
    const NPBucket* tab = nullptr;
    const int64_t* pays = nullptr;
    unsigned long long* cnt = nullptr;
    uint64_t table_bytes = 0;
};

// What these forms refuse before they size anything: the hash, 2^32 tuples a side.
int np_limits(phj_ctx* c, const phj_join_params* p) {
    if (p->hash != PHJ_HASH_XXH3 && p->hash != PHJ_HASH_MURMUR3)
        return set_err(c, PHJ_ERR_INVALID, "unknown hash function");
    if (c->side[PHJ_SIDE_BUILD].n >= (1ull << 32)) return set_err(c, PHJ_ERR_RANGE, "build side above 2^32 tuples");
    if (c->side[PHJ_SIDE_PROBE].n >= (1ull << 32)) return set_err(c, PHJ_ERR_RANGE, "probe side above 2^32 tuples");
    return PHJ_OK;
}

// The table built (np_build), the probe's grid and arguments. Every form calls
// np_limits itself, before the workspace it sizes ahead of the build, and
// clears the count word after this if its probe counts there.
int np_setup(phj_ctx* c, const phj_join_params* p, bool slots32, PaySrc pay, NPJoin& j) {
    const SideState& S = c->side[PHJ_SIDE_PROBE];
    PHJ_TRY(np_build(c, p, slots32, j.g, &j.e0, pay));
    PHJ_TRY(mark(c, &j.e1));
    j.grid = static_cast<uint32_t>(std::min<uint64_t>((S.n + 4 * kBlock - 1) / (4 * kBlock), 8192));
    j.S_rel = reinterpret_cast<const longlong2*>(S.rel);
    j.tab = static_cast<const NPBucket*>(c->np_tab.p);
    j.pays = static_cast<const int64_t*>(c->np_pays.p);
    j.cnt = static_cast<unsigned long long*>(c->count.p);
    j.table_bytes = static_cast<uint64_t>(j.g.nb) * 64;
    return PHJ_OK;
}

// phj_index_build (phj_lookup.h): np_build's schedule over buckets of five
// {code, row} entries. R is partitioned by region with its row numbers as the
// payload (keys only, nothing packed), one workgroup per region finds or
// claims in LDS, the overflow list follows with device atomics. The table is
// the index's own allocation; the partition and the overflow list are the
// context's workspace and are free again when the call returns.
int index_geometry(phj_ctx* c, uint64_t rows, double table_ratio, NPHome& g) {
    // (a region of more than kIxRegionBuckets buckets would need 2^22 regions of them: beyond 2^32 buckets)
    return table_geometry(c, std::max<uint64_t>(1, rows), table_ratio, kIxSlots, kIxRegionBuckets, kIxRegionBuckets,
                          "phj_index_build: ", g);
}

int index_build(phj_ctx* c, const phj_join_params* p, uint32_t flags, phj_index** out, phj_join_result* r) {
    const char* what = "phj_index_build";
    if (!c || !out || !r) return PHJ_ERR_INVALID;
    *out = nullptr;
    if (c->group) return set_err(c, PHJ_ERR_STATE, std::string(what) + ": single-device contexts only");
    if (!p) return set_err(c, PHJ_ERR_INVALID, "null params");
    if (flags & ~static_cast<uint32_t>(PHJ_INDEX_ORDINALS)) return set_err(c, PHJ_ERR_INVALID, std::string(what) + ": unknown flags");
    const bool ordinals = (flags & PHJ_INDEX_ORDINALS) != 0;
    if (p->algo != PHJ_ALGO_NO_PARTITIONING && p->algo != PHJ_ALGO_RADIX)
        return set_err(c, PHJ_ERR_INVALID, "Unrecognized join algorithm");
    if (p->hash != PHJ_HASH_XXH3 && p->hash != PHJ_HASH_MURMUR3) return set_err(c, PHJ_ERR_INVALID, "unknown hash function");
    if (p->algo == PHJ_ALGO_RADIX) {   // the usual validation; the plan itself is not used
        Plan asked;
        PHJ_TRY(make_plan(c, p, asked));
    }
    SideState& R = c->side[PHJ_SIDE_BUILD];
    if (!R.rel && !R.columns && R.n > 0) return set_err(c, PHJ_ERR_STATE, "relation not bound");
    if (R.n >= (1ull << 30)) return set_err(c, PHJ_ERR_RANGE, std::string(what) + ": build side of 2^30 rows or more");
    NPHome g{};
    PHJ_TRY(index_geometry(c, R.n, p->table_ratio, g));
    PHJ_TRY(begin_call(c));
    std::memset(r, 0, sizeof(*r));
    const uint32_t nb = g.nb;
    // ordinals: one bit per build row in 32-bit words, rounded to 16 B so that the rank array behind it scans vectorised
    const uint64_t ord_words = ((R.n + 31) / 32 + 3) & ~3ull;
    if (R.n > 0) {   // the workspace first: a grow synchronises, and nothing of the index exists yet
        PHJ_TRY(ensure(c, c->count, 32));
        // (ordinals: the bitmap and the rank array take the overflow list's place once that pass is done)
        PHJ_TRY(ensure(c, c->np_ovf, std::max<uint64_t>(R.n * 16, ordinals ? 2 * ord_words * 4 : 0)));
        PHJ_TRY(ensure(c, c->np_ovfb, R.n * 4));
        PHJ_TRY(ensure(c, c->np_ovfn, 4));
        if (ordinals) PHJ_TRY(ensure(c, c->scan_partials, (ord_words + kScanBlockElems - 1) / kScanBlockElems * 4));
    }
    phj_index* ix = new phj_index();
    ix->owner = c;
    ix->flags = flags;
    ix->g = g;
    ix->hk = p->hash;
    ix->seed = p->hash_seed;
    ix->rows = R.n;
    ix->bytes = static_cast<size_t>(nb) * sizeof(IxBucket);
    auto fail = [&](int rc) {
        if (ix->tab) (void)hipFree(ix->tab);
        if (ix->first_rows) (void)hipFree(ix->first_rows);
        delete ix;
        return rc;
    };
    {
        void* mem = nullptr;
        const hipError_t e = hipMalloc(&mem, ix->bytes);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(set_err(c, PHJ_ERR_NOMEM, "hipMalloc(" + std::to_string(ix->bytes) + "): " + hipGetErrorString(e)));
        }
        ix->tab = static_cast<IxBucket*>(mem);
    }
#define PHJ_IX(expr)                          \
    do {                                      \
        const int rc_ix_ = (expr);            \
        if (rc_ix_ != PHJ_OK) return fail(rc_ix_); \
    } while (0)
    auto hip = [&](hipError_t e, const char* call) {
        return e == hipSuccess ? PHJ_OK : set_err(c, PHJ_ERR_HIP, std::string(call) + ": " + hipGetErrorString(e));
    };
    auto launched = [&](const char* kernel) {   // PHJ_LAUNCHED, through fail()
        c->since_ev++;
        return hip(hipGetLastError(), (std::string("launch ") + kernel).c_str());
    };
    if (c->poison >= 0)   // (test hook) the region build writes every bucket before anything reads one
        PHJ_IX(hip(hipMemsetAsync(ix->tab, c->poison, ix->bytes, c->ks), "hipMemsetAsync"));
    const void* kfn = with_hash(p->hash, [&](auto h) {
        return reinterpret_cast<const void*>(&k_ix_lookup<decltype(h)::value, 1>);   // (both strides share a resource shape)
    });
    ix->max_wgs = static_cast<uint32_t>(occupancy_or(kfn, 256, 0, 4)) * static_cast<uint32_t>(std::max(1, c->num_cus));
    if (ordinals) {
        const void* afn = with_hash(p->hash, [&](auto h) {
            return reinterpret_cast<const void*>(&k_ix_accumulate<decltype(h)::value, 1>);
        });
        ix->acc_wgs = static_cast<uint32_t>(occupancy_or(afn, 256, 0, 4)) * static_cast<uint32_t>(std::max(1, c->num_cus));
    }
    if (R.n == 0) {   // a valid index over nothing: every bucket empty, every lookup misses
        PHJ_IX(hip(hipMemsetAsync(ix->tab, 0, ix->bytes, c->ks), "hipMemsetAsync"));
        PHJ_IX(hip(hipStreamSynchronize(c->ks), "hipStreamSynchronize"));
        c->indexes.push_back(ix);
        *out = ix;
        return PHJ_OK;
    }
    Plan rp;
    PHJ_IX(region_plan(c, p, g.rbits, rp));
    hipEvent_t e0, e1;
    PHJ_IX(mark(c, &e0));
    PHJ_IX(partition_side(c, PHJ_SIDE_BUILD, rp, false, nullptr, PaySrc::RowNumber));
    const phj_partitioned& v = R.view;
    auto* cnt = static_cast<unsigned long long*>(c->count.p);
    auto* ovn = static_cast<uint32_t*>(c->np_ovfn.p);
    auto* ov = static_cast<ulonglong2*>(c->np_ovf.p);
    auto* ovb = static_cast<uint32_t*>(c->np_ovfb.p);
    // algorithmic bytes: the partitioned keys and rows read (16 B per tuple), every bucket written
    PHJ_IX(timer_begin(c, "index.build", R.n * 16 + static_cast<uint64_t>(nb) * 64));
    PHJ_IX(hip(hipMemsetAsync(cnt, 0, 16, c->ks), "hipMemsetAsync"));
    PHJ_IX(hip(hipMemsetAsync(ovn, 0, 4, c->ks), "hipMemsetAsync"));
    {
        const size_t lds = static_cast<size_t>(g.nbr) * sizeof(IxBucket);
        IxBucket* tab = ix->tab;
        with_hash(p->hash, [&](auto h) {
            hipLaunchKernelGGL((k_ix_build_region<decltype(h)::value>), dim3(1u << g.rbits), dim3(kBlock), lds, c->ks, v.keys,
                               v.payloads, v.bounds, g, tab, p->hash_seed, ovn, ov, ovb, cnt);
        });
        PHJ_IX(launched("k_ix_build_region"));
        hipLaunchKernelGGL(k_ix_build_overflow, dim3(64), dim3(kBlock), 0, c->ks, ovn, ov, ovb, tab, nb, cnt);
        PHJ_IX(launched("k_ix_build_overflow"));
    }
    PHJ_IX(timer_end(c));
    if (!ordinals) PHJ_IX(mark(c, &e1));
    unsigned long long h[2] = {0, 0};   // {distinct codes, the overflow pass gave up on a tuple}
    PHJ_IX(hip(hipMemcpyAsync(h, cnt, sizeof(h), hipMemcpyDeviceToHost, c->ks), "hipMemcpyAsync"));
    PHJ_IX(hip(hipStreamSynchronize(c->ks), "hipStreamSynchronize"));
    if (h[1]) return fail(set_err(c, PHJ_ERR_STATE, std::string(what) + ": the table had no room for a key"));
    if (ordinals) {   // first_rows has `distinct` entries: allocated once that is known, then the four passes
        c->since_ev++;   // (the copy back and the wait lie between the two timers: no shared boundary event)
        const uint64_t distinct = h[0];
        const size_t fbytes = static_cast<size_t>(distinct) * sizeof(int64_t);
        void* mem = nullptr;
        const hipError_t e = hipMalloc(&mem, fbytes);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(set_err(c, PHJ_ERR_NOMEM, "hipMalloc(" + std::to_string(fbytes) + "): " + hipGetErrorString(e)));
        }
        ix->first_rows = static_cast<int64_t*>(mem);
        ix->bytes += fbytes;
        if (c->poison >= 0) PHJ_IX(hip(hipMemsetAsync(ix->first_rows, c->poison, fbytes, c->ks), "hipMemsetAsync"));
        const uint32_t rows = static_cast<uint32_t>(R.n), words = static_cast<uint32_t>(ord_words);
        uint32_t* bitmap = static_cast<uint32_t*>(c->np_ovf.p);   // (the overflow pass is done with it)
        uint32_t* rank = bitmap + words;
        // algorithmic bytes: the row words of every bucket read twice and written once (a 32-B half line each
        // time), the bitmap cleared, written, and read three times, the rank written, scanned (read twice,
        // written once) and read twice, first_rows written
        PHJ_IX(timer_begin(c, "index.ordinals", static_cast<uint64_t>(nb) * 96 + static_cast<uint64_t>(words) * (20 + 24) + fbytes));
        PHJ_IX(hip(hipMemsetAsync(bitmap, 0, static_cast<size_t>(words) * 4, c->ks), "hipMemsetAsync"));
        const uint32_t sgrid = static_cast<uint32_t>((static_cast<uint64_t>(nb) * 8 + kBlock - 1) / kBlock);
        hipLaunchKernelGGL(k_ix_ord_mark, dim3(sgrid), dim3(kBlock), 0, c->ks, ix->tab, nb, rows, bitmap);
        PHJ_IX(launched("k_ix_ord_mark"));
        hipLaunchKernelGGL(k_ix_ord_popc, dim3((words + kBlock - 1) / kBlock), dim3(kBlock), 0, c->ks, bitmap, words, rank);
        PHJ_IX(launched("k_ix_ord_popc"));
        PHJ_IX(scan_u32(c, rank, words, 1, words));
        hipLaunchKernelGGL(k_ix_ord_first, dim3((rows + kBlock - 1) / kBlock), dim3(kBlock), 0, c->ks, bitmap, rank, rows,
                           ix->first_rows, distinct);
        PHJ_IX(launched("k_ix_ord_first"));
        hipLaunchKernelGGL(k_ix_ord_apply, dim3(sgrid), dim3(kBlock), 0, c->ks, ix->tab, nb, rows, bitmap, rank);
        PHJ_IX(launched("k_ix_ord_apply"));
        PHJ_IX(timer_end(c));
        PHJ_IX(mark(c, &e1));
        PHJ_IX(hip(hipStreamSynchronize(c->ks), "hipStreamSynchronize"));
    }
#undef PHJ_IX
    ix->distinct = h[0];
    r->matches = h[0];
    r->partition_ms = 0;
    r->build_ms = elapsed(c, e0, e1);
    r->probe_ms = 0;
    r->total_ms = elapsed(c, e0, e1);
    r->num_partitions = 0;
    const int rc = fill_timers(c, r);
    if (rc != PHJ_OK) return fail(rc);
    for (uint32_t i = 0; i < r->num_timers; i++) r->algorithmic_bytes += r->timer_bytes[i];   // R's passes and the build
    c->indexes.push_back(ix);
    *out = ix;
    return PHJ_OK;
}

// phj_index_lookup: one launch on the context's stream and nothing else: no
// event, no allocation, no copy back, no synchronisation.
// codes: phj_index_encode, the ordinals of an ordinal index in place of rows.
int index_lookup(phj_ctx* c, const phj_index* ix, const int64_t* keys, uint32_t key_stride, uint64_t n, int64_t* out_rows,
                 uint8_t* out_found, unsigned long long* dev_found_count, bool codes = false) {
    const char* what = codes ? "phj_index_encode" : "phj_index_lookup";
    if (!c || !ix) return PHJ_ERR_INVALID;
    if (c->group) return set_err(c, PHJ_ERR_STATE, std::string(what) + ": single-device contexts only");
    if (ix->owner != c) return set_err(c, PHJ_ERR_INVALID, std::string(what) + ": the index belongs to another context");
    if (codes && !(ix->flags & PHJ_INDEX_ORDINALS)) return set_err(c, PHJ_ERR_STATE, std::string(what) + ": index built without ordinals");
    if (key_stride != 1 && key_stride != 2)
        return set_err(c, PHJ_ERR_INVALID, std::string(what) + ": key_stride must be 1 (a key column) or 2 (the ids of tuples)");
    if (n == 0) return PHJ_OK;
    if (!keys || !out_rows) return set_err(c, PHJ_ERR_INVALID, std::string(what) + ": null keys or out_rows");
    if ((reinterpret_cast<uintptr_t>(keys) | reinterpret_cast<uintptr_t>(out_rows) |
         reinterpret_cast<uintptr_t>(dev_found_count)) & 7)
        return set_err(c, PHJ_ERR_INVALID, std::string(what) + ": keys, out_rows and the counter need 8-byte alignment");
    (void)hipGetLastError();
    PHJ_HIP(c, hipSetDevice(c->device));
    IxLookupArgs a{};
    a.keys = keys;
    a.n = n;
    a.tab = ix->tab;
    a.g = ix->g;
    a.seed = ix->seed;
    a.rows = out_rows;
    a.found = out_found;
    a.count = dev_found_count;
    a.first = ix->first_rows;
    const bool ord = (ix->flags & PHJ_INDEX_ORDINALS) != 0;
    const void* kfn = with_hash(ix->hk, [&](auto h) {
        constexpr int HK = decltype(h)::value;
        auto pick = [&](auto m) {
            constexpr IxMode M = decltype(m)::value;
            return key_stride == 1 ? reinterpret_cast<const void*>(&k_ix_lookup<HK, 1, M>)
                                   : reinterpret_cast<const void*>(&k_ix_lookup<HK, 2, M>);
        };
        if (!ord) return pick(std::integral_constant<IxMode, IxMode::Rows>{});
        if (codes) return pick(std::integral_constant<IxMode, IxMode::Codes>{});
        return pick(std::integral_constant<IxMode, IxMode::RowsVia>{});
    });
    const uint64_t per = 256ull * kIxItems;
    const uint32_t grid = static_cast<uint32_t>(std::max<uint64_t>(1, std::min<uint64_t>((n + per - 1) / per, ix->max_wgs)));
    void* kargs[] = {&a};
    PHJ_HIP(c, hipLaunchKernel(kfn, dim3(grid), dim3(256), kargs, 0, c->stream));
    PHJ_LAUNCHED(c, "k_ix_lookup");
    return PHJ_OK;
}

// phj_index_accumulate: enqueue-only like the lookup. One launch per 2^31 keys
// (k_ix_accumulate's cache counts in 32 bits between its flushes).
int index_accumulate(phj_ctx* c, const phj_index* ix, const int64_t* keys, uint32_t key_stride, const int64_t* values,
                     uint32_t value_stride, uint64_t n, unsigned long long* counts, int64_t* sums,
                     unsigned long long* missing) {
    const char* what = "phj_index_accumulate";
    if (!c || !ix) return PHJ_ERR_INVALID;
    if (c->group) return set_err(c, PHJ_ERR_STATE, std::string(what) + ": single-device contexts only");
    if (ix->owner != c) return set_err(c, PHJ_ERR_INVALID, std::string(what) + ": the index belongs to another context");
    if (!(ix->flags & PHJ_INDEX_ORDINALS)) return set_err(c, PHJ_ERR_STATE, std::string(what) + ": index built without ordinals");
    if (key_stride != 1 && key_stride != 2)
        return set_err(c, PHJ_ERR_INVALID, std::string(what) + ": key_stride must be 1 (a key column) or 2 (the ids of tuples)");
    if ((values == nullptr) != (sums == nullptr))
        return set_err(c, PHJ_ERR_INVALID, std::string(what) + ": dev_values and dev_sums go together");
    if (values && value_stride != 1 && value_stride != 2)
        return set_err(c, PHJ_ERR_INVALID, std::string(what) + ": value_stride must be 1 or 2");
    if (n == 0) return PHJ_OK;
    if (!keys || !counts) return set_err(c, PHJ_ERR_INVALID, std::string(what) + ": null keys or dev_counts");
    if ((reinterpret_cast<uintptr_t>(keys) | reinterpret_cast<uintptr_t>(values) | reinterpret_cast<uintptr_t>(counts) |
         reinterpret_cast<uintptr_t>(sums) | reinterpret_cast<uintptr_t>(missing)) & 7)
        return set_err(c, PHJ_ERR_INVALID, std::string(what) + ": every pointer needs 8-byte alignment");
    (void)hipGetLastError();
    PHJ_HIP(c, hipSetDevice(c->device));
    const void* kfn = with_hash(ix->hk, [&](auto h) {
        constexpr int HK = decltype(h)::value;
        return key_stride == 1 ? reinterpret_cast<const void*>(&k_ix_accumulate<HK, 1>)
                               : reinterpret_cast<const void*>(&k_ix_accumulate<HK, 2>);
    });
    const uint64_t per = 256ull * kIxItems;
    for (uint64_t off = 0; off < n; off += kIxAccLaunchKeys) {
        IxAccArgs a{};
        a.n = std::min<uint64_t>(kIxAccLaunchKeys, n - off);
        a.keys = keys + off * key_stride;
        a.tab = ix->tab;
        a.g = ix->g;
        a.seed = ix->seed;
        a.values = values ? values + off * value_stride : nullptr;
        a.vstride = value_stride;
        a.counts = counts;
        a.sums = reinterpret_cast<unsigned long long*>(sums);
        a.missing = missing;
        const uint32_t grid = static_cast<uint32_t>(std::max<uint64_t>(1, std::min<uint64_t>((a.n + per - 1) / per, ix->acc_wgs)));
        void* kargs[] = {&a};
        PHJ_HIP(c, hipLaunchKernel(kfn, dim3(grid), dim3(256), kargs, 0, c->stream));
        PHJ_LAUNCHED(c, "k_ix_accumulate");
    }
    return PHJ_OK;
}

// marks != nullptr: the probe also writes, per probe tuple, its match's payload
// slot (phj_join_materialize)
int join_nopart(phj_ctx* c, const phj_join_params* p, phj_join_result* r, uint32_t* marks = nullptr) {
    SideState& R = c->side[PHJ_SIDE_BUILD];
    SideState& S = c->side[PHJ_SIDE_PROBE];
    if (p->hash != PHJ_HASH_XXH3 && p->hash != PHJ_HASH_MURMUR3)
        return set_err(c, PHJ_ERR_INVALID, "unknown hash function");
    if (R.n == 0)  // LinearProbing.hpp:295-299
        return set_err(c, PHJ_ERR_INVALID,
                       "LinearProbingHashTable::LinearProbingHashTable: numberOfObjects must be greater than zero.");
    if (R.n >= (1ull << 32)) return set_err(c, PHJ_ERR_RANGE, "build side above 2^32 tuples");
    if (!marks && R.n < (1ull << 30)) return join_nopart_ct(c, p, r);
    NPHome g{};
    hipEvent_t e0 = nullptr, e1, e2;
    PHJ_TRY(np_build(c, p, marks != nullptr, g, &e0));
    if (c->dry) return PHJ_OK;
    const uint32_t nb = g.nb;
    PHJ_TRY(mark(c, &e1));
    PHJ_HIP(c, hipMemsetAsync(c->count.p, 0, 8, c->ks));
    if (S.n > 0) {
        const uint64_t per = static_cast<uint64_t>(kBlock) * 4;
        const uint32_t pg = static_cast<uint32_t>(std::min<uint64_t>((S.n + per - 1) / per, 8192));
        PHJ_TRY(timer_begin(c, "np.probe", S.n * 16 + static_cast<uint64_t>(nb) * 64));
        const auto* S_rel = reinterpret_cast<const longlong2*>(S.rel);
        const auto* tab = static_cast<const NPBucket*>(c->np_tab.p);
        auto* cnt = static_cast<unsigned long long*>(c->count.p);
        // (the count takes join_nopart_ct below 2^30 build tuples; this bucket
        // probe serves larger build sides and, with marks, the materialised join)
        if (marks) {
            const uint32_t mg = static_cast<uint32_t>(std::min<uint64_t>((S.n + 4 * kBlock - 1) / (4 * kBlock), 8192));
            with_hash(p->hash, [&](auto h) {
                hipLaunchKernelGGL((k_np_probe_mark<decltype(h)::value>), dim3(mg), dim3(kBlock), 0, c->ks, S_rel, S.n,
                                   tab, g, p->hash_seed, marks, cnt);
            });
        } else {
            with_hash(p->hash, [&](auto h) {
                hipLaunchKernelGGL((k_np_probe<decltype(h)::value, 4, 1>), dim3(pg), dim3(kBlock), 0, c->ks, S_rel, S.n,
                                   tab, g, p->hash_seed, cnt);
            });
        }
        PHJ_LAUNCHED(c, "k_np_probe");
        PHJ_TRY(timer_end(c));
    }
    PHJ_TRY(mark(c, &e2));
    uint64_t m = 0;
    PHJ_TRY(get_count(c, &m));
    r->matches = m;
    r->algorithmic_bytes = R.n * 32 + S.n * 16 + static_cast<uint64_t>(nb) * 64;
    return np_times(c, e0, e1, e2, r);
}

int check_side(phj_ctx* c, int side) {
    if (!c) return PHJ_ERR_INVALID;
    (void)hipGetLastError();  // drop a stale error left by code outside this library
    if (side != PHJ_SIDE_BUILD && side != PHJ_SIDE_PROBE)
        return set_err(c, PHJ_ERR_INVALID, "side must be PHJ_SIDE_BUILD or PHJ_SIDE_PROBE");
    return PHJ_OK;
}

void drop_relation(phj_ctx* c, int side) {
    SideState& S = c->side[side];
    S.rel = nullptr;
    S.n = 0;
    S.partitioned = false;
    // (a columnar binding and its packed copy go with it; the buffers stay, grow-only)
    S.columns = S.cols_owned = S.packed = false;
    S.ckeys = S.cpays = nullptr;
}

// The calls without a column form run on tuples: a side bound as columns is
// packed once into a ctx-owned tuple buffer (k_pack_columns; payload 0 for a
// key column alone) that stays until the side is rebound, and S.rel names it.
// The call that packs records it as `S.pack` / `R.pack`, 16 B read and 16 B
// written per tuple. need_pay: the call's result holds payloads, so a key
// column alone is refused before anything is launched. phj_prepare (dry) only
// sizes the buffer.
int need_tuples(phj_ctx* c, int side, bool need_pay, const char* what) {
    SideState& S = c->side[side];
    if (!S.columns) return PHJ_OK;
    if (need_pay && !S.cpays && S.n > 0)
        return set_err(c, PHJ_ERR_STATE, std::string(what) + ": payload column not bound on the " +
                                             (side == PHJ_SIDE_BUILD ? "build" : "probe") + " side");
    if (S.packed || S.n == 0) return PHJ_OK;
    PHJ_TRY(ensure(c, S.pack, S.n * sizeof(phj_tuple)));
    if (c->dry) return PHJ_OK;
    PHJ_TRY(timer_begin(c, side == PHJ_SIDE_BUILD ? "R.pack" : "S.pack", S.n * 32));
    const uint32_t g = static_cast<uint32_t>(std::min<uint64_t>((S.n + kBlock - 1) / kBlock, 65536));
    hipLaunchKernelGGL(k_pack_columns, dim3(g), dim3(kBlock), 0, c->ks, S.ckeys, S.cpays, S.n, static_cast<longlong2*>(S.pack.p));
    PHJ_LAUNCHED(c, "k_pack_columns");
    PHJ_TRY(timer_end(c));
    S.rel = static_cast<const phj_tuple*>(S.pack.p);
    S.packed = true;
    return PHJ_OK;
}

// Both sides; the payload check of both comes before either is packed.
int need_tuples_both(phj_ctx* c, bool need_pay, const char* what) {
    for (int side : {PHJ_SIDE_BUILD, PHJ_SIDE_PROBE}) {
        const SideState& S = c->side[side];
        if (need_pay && S.columns && !S.cpays && S.n > 0) return need_tuples(c, side, true, what);
    }
    PHJ_TRY(need_tuples(c, PHJ_SIDE_BUILD, need_pay, what));
    return need_tuples(c, PHJ_SIDE_PROBE, need_pay, what);
}

uint64_t partition_bytes(const Plan& pl, uint64_t n) {
    // hist (16 B AoS read) + scatter (16 read + 16 write); pass 2: hist 8 + scatter 32
    return n * (16 + 32) + (pl.npass == 2 ? n * (8 + 32) : 0);
}

// Rows of a marked probe (phj_mat.h): block counts, exclusive scan, write.
int mat_compact(phj_ctx* c, uint64_t nS, const longlong2* s_aos, const int64_t* sk, const int64_t* sp,
                const int64_t* rpay) {
    const uint32_t nblk = static_cast<uint32_t>((nS + kMatBlock - 1) / kMatBlock);
    PHJ_TRY(ensure(c, c->mat_cnt, (static_cast<size_t>(nblk) + 1) * 4));
    PHJ_TRY(ensure(c, c->mat_rows, std::max<uint64_t>(1, nS) * sizeof(JoinedRow)));
    auto* cnt = static_cast<uint32_t*>(c->mat_cnt.p);
    const auto* mark = static_cast<const uint32_t*>(c->mat_mark.p);
    PHJ_TRY(timer_begin(c, "mat.write", nS * 20 + static_cast<uint64_t>(nS) * 4));
    PHJ_HIP(c, hipMemsetAsync(cnt, 0, (static_cast<size_t>(nblk) + 1) * 4, c->ks));
    if (nblk) {
        hipLaunchKernelGGL(k_mat_count, dim3(nblk), dim3(kBlock), 0, c->ks, mark, nS, cnt);
        PHJ_LAUNCHED(c, "k_mat_count");
    }
    PHJ_TRY(scan_u32(c, cnt, nblk + 1, 1, nblk + 1));
    if (nblk) {
        hipLaunchKernelGGL(k_mat_write, dim3(nblk), dim3(kBlock), 0, c->ks, mark, nS, s_aos, sk, sp, rpay, cnt,
                           static_cast<JoinedRow*>(c->mat_rows.p));
        PHJ_LAUNCHED(c, "k_mat_write");
    }
    return timer_end(c);
}

// The radix forms of the materialised join and of the row and aggregate joins
// (the fused per-partition LDS join of both sides fully partitioned, SoA):
// what they share before their first join kernel (fused_setup, fused_items)
// and at their end (fused_times).
struct FusedJoin {
    Plan pl;
    uint32_t requested = 0;   // partitions asked for (pl may be refined)
    uint64_t nS = 0;          // partitioned probe tuples: mat_mark has one word each
    hipEvent_t t0 = nullptr, t1 = nullptr;   // around the partitioning
    FusedArgs fa{};
    uint32_t grid = 0;
};

// Plan, precondition ("<what> needs ..."), both sides partitioned, the
// workspace sized, the count cleared, the join kernels' arguments and grid.
int fused_setup(phj_ctx* c, const phj_join_params* p, const char* what, FusedJoin& j, PaySrc pay = PaySrc::Bound) {
    PHJ_TRY(make_plan(c, p, j.pl));
    SideState& R = c->side[PHJ_SIDE_BUILD];
    SideState& S = c->side[PHJ_SIDE_PROBE];
    j.requested = j.pl.Ppad;
    refine_plan(c, j.pl, R.n);
    const uint32_t P = j.pl.Ppad;
    if (!c->tune.fused || (R.n + P - 1) / P * 3 > static_cast<uint64_t>(kFusedTcap) * 2)
        return set_err(c, PHJ_ERR_INVALID, std::string(what) + " needs the fused LDS join (PHJ_FUSED, PHJ_SUBPART)");
    PHJ_TRY(mark(c, &j.t0));
    PHJ_TRY(partition_side(c, PHJ_SIDE_PROBE, j.pl, false, nullptr, pay));
    PHJ_TRY(partition_side(c, PHJ_SIDE_BUILD, j.pl, false, nullptr, pay));
    PHJ_TRY(mark(c, &j.t1));
    j.nS = S.view.n;
    const size_t nslots = j.nS / kFusedChunk + P + 1;
    PHJ_TRY(ensure(c, c->fitems, nslots * sizeof(FusedItem)));
    PHJ_TRY(ensure(c, c->count, 32));
    PHJ_TRY(ensure(c, c->mat_mark, j.nS * 4));
    PHJ_HIP(c, hipMemsetAsync(c->count.p, 0, 8, c->ks));
    FusedArgs& fa = j.fa;
    fa.L.nseg = 1;
    fa.L.P = P;
    fa.L.seg[0].keys = R.view.keys;
    fa.L.seg[0].pays = R.view.payloads;
    fa.L.seg[0].bounds = R.view.bounds;
    fa.skeys = S.view.keys;
    fa.sbounds = S.view.bounds;
    fa.items = static_cast<const FusedItem*>(c->fitems.p);
    fa.nitems = static_cast<uint32_t>(nslots - 1);
    fa.count = static_cast<unsigned long long*>(c->count.p);
    fa.seed = j.pl.seed;
    j.grid = chip_grid(c, (nslots + kWaves - 1) / kWaves, 4);
    return PHJ_OK;
}

// The work items of the join kernels, written inside the first one's timer.
int fused_work_items(phj_ctx* c, const FusedJoin& j) {
    hipLaunchKernelGGL(k_fused_items, dim3((j.fa.L.P + kWaves - 1) / kWaves), dim3(kBlock), 0, c->ks, j.fa.sbounds,
                       j.fa.L.P, static_cast<FusedItem*>(c->fitems.p));
    PHJ_LAUNCHED(c, "k_fused_items");
    return PHJ_OK;
}

// Opens the first join kernel's timer (it reads the build keys and the probe
// keys and writes a word per probe tuple) with the work items inside it.
int fused_items(phj_ctx* c, const char* timer, const FusedJoin& j) {
    PHJ_TRY(timer_begin(c, timer, c->side[PHJ_SIDE_BUILD].n * 8 + j.nS * 12));
    return fused_work_items(c, j);
}

// p1: the event behind the join's last kernel.
int fused_times(phj_ctx* c, const FusedJoin& j, hipEvent_t p1, phj_join_result* r) {
    r->partition_ms = elapsed(c, j.t0, j.t1);
    r->probe_ms = elapsed(c, j.t1, p1);
    r->total_ms = elapsed(c, j.t0, p1);
    return fill_timers(c, r);
}

int join_radix_mark(phj_ctx* c, const phj_join_params* p, phj_join_result* r) {
    FusedJoin j;
    PHJ_TRY(fused_setup(c, p, "materialised radix join", j));
    const SideState& R = c->side[PHJ_SIDE_BUILD];
    const SideState& S = c->side[PHJ_SIDE_PROBE];
    auto* mk = static_cast<uint32_t*>(c->mat_mark.p);
    PHJ_HIP(c, hipMemsetAsync(mk, 0xff, std::max<uint64_t>(1, j.nS) * 4, c->ks));
    PHJ_TRY(fused_items(c, "mat.join", j));
    with_hash(j.pl.hk, [&](auto h) {
        hipLaunchKernelGGL(k_join_fused_mark<decltype(h)::value>, dim3(j.grid), dim3(kBlock), 0, c->ks, j.fa, mk);
    });
    PHJ_LAUNCHED(c, "k_join_fused_mark");
    PHJ_TRY(timer_end(c));
    PHJ_TRY(mat_compact(c, j.nS, nullptr, S.view.keys, S.view.payloads, R.view.payloads));
    hipEvent_t p1;
    PHJ_TRY(mark(c, &p1));
    uint64_t m = 0;
    PHJ_TRY(get_count(c, &m));
    r->matches = m;
    r->num_partitions = j.requested;
    r->algorithmic_bytes = partition_bytes(j.pl, R.n) + partition_bytes(j.pl, S.n) + R.n * 8 + j.nS * 12 + m * 24;
    return fused_times(c, j, p1, r);
}

// ---- the inner join (phj_inner.h): count, offsets, emit ----

constexpr uint64_t kInnerRowLimit = 1ull << 32;   // rows are addressed with 32 bits (scan_u32)

// Pass 2 of the inner join: pairs[0, nS) (mat_mark) -> each probe tuple's
// first row, in place. Launched inside the caller's emit timer.
int inner_offsets(phj_ctx* c, uint64_t nS) {
    const uint32_t nblk = static_cast<uint32_t>((nS + kMatBlock - 1) / kMatBlock);
    auto* cnt = static_cast<uint32_t*>(c->mat_cnt.p);
    auto* pairs = static_cast<uint32_t*>(c->mat_mark.p);
    PHJ_HIP(c, hipMemsetAsync(cnt, 0, (static_cast<size_t>(nblk) + 1) * 4, c->ks));
    hipLaunchKernelGGL(k_inner_blocksum, dim3(nblk), dim3(kBlock), 0, c->ks, pairs, nS, cnt);
    PHJ_LAUNCHED(c, "k_inner_blocksum");
    PHJ_TRY(scan_u32(c, cnt, nblk + 1, 1, nblk + 1));
    hipLaunchKernelGGL(k_inner_prefix, dim3(nblk), dim3(kBlock), 0, c->ks, pairs, nS, cnt);
    PHJ_LAUNCHED(c, "k_inner_prefix");
    return PHJ_OK;
}

// Bytes the count pass must move, beyond partitioning / the table build
// (DESIGN.md §Inner join): it reads the probe keys and the build keys and
// writes pairs[]. (The emit pass: rows_emit_bytes.)
uint64_t inner_count_bytes(uint64_t nR, uint64_t nS) { return nR * 8 + nS * (8 + 4); }

// The two index columns of n rows in the row buffer (phj_ctx::idx_n).
IndexSink index_sink(phj_ctx* c, uint64_t n) {
    int64_t* base = static_cast<int64_t*>(c->mat_rows.p);
    return IndexSink{base, base + n};
}

// Where the emitting kernels store: the row buffer as 24-B rows, or as the two
// index columns (phj_join_indices). f(sink) with the one in use, so that a
// kernel template over the sink is named once per launch site.
struct RowSinks {
    JoinedRow* rows;
    IndexSink index;
};
template <class F>
void with_sink(bool index, const RowSinks& s, F f) {
    if (index) f(s.index);
    else f(s.rows);
}

// ---- the join form: what the row and aggregate joins run on ----

// A join set up in its NoPartitioning form (np_setup: the bucket table built,
// S probed where it is bound) or its radix form (fused_setup: both sides fully
// partitioned, SoA, for the per-partition LDS join), as the passes behind it
// see either: the probe side in storage order (pairs[] has one word per
// tuple), the build storage that hit flags and accumulators index, the bytes
// and the report of what ran so far.
struct JoinForm {
    NPJoin np;      // NoPartitioning (tab != nullptr)
    FusedJoin fu;   // radix
    int hk = 0;
    uint64_t seed = 0;
    uint64_t nS = 0;
    const longlong2* s_aos = nullptr;             // NoPartitioning: AoS tuples
    const int64_t *sk = nullptr, *sp = nullptr;   // radix: the partitioned columns
    uint64_t nF = 0;                              // elements of the build storage
    const NPBucket* tab = nullptr;                // NoPartitioning: the table (keys), rp = np_pays
    const int64_t *rk = nullptr, *rp = nullptr;
    // phj_join_indices: the payloads the join carries are row numbers (sp, rp;
    // NoPartitioning: s_aos and sk are null and a probe tuple's number is its
    // position) and the emit pass stores into the two index columns.
    // NoPartitioning reads S for its keys alone (k_np_inner KEYS): keys = 1 its
    // key column itself, 2 its tuples' ids, 0 whole tuples.
    bool index = false;
    int keys = 0;
    const longlong2* s_probe = nullptr;
    // what a pass reads of the build side (its keys, or the bucket table), the
    // table alone, the count pass, and everything before the first join kernel
    uint64_t build_bytes = 0, table_bytes = 0, count_bytes = 0, front_bytes = 0;
    uint32_t num_partitions = 0;
};

// The limits, the workspace that is sized ahead of the build, then the form.
// what: the radix form's name in its precondition ("<what> needs ...").
// pairs: the join counts into pairs[] and the count words {pairs, probe_only,
// build_only} (the first one cleared here); the aggregates have words of their own.
int form_setup(phj_ctx* c, const phj_join_params* p, const char* what, bool pairs, bool index, JoinForm& J) {
    const SideState& R = c->side[PHJ_SIDE_BUILD];
    const SideState& S = c->side[PHJ_SIDE_PROBE];
    const PaySrc pay = index ? PaySrc::RowNumber : PaySrc::Bound;
    J.index = index;
    if (p->algo == PHJ_ALGO_NO_PARTITIONING) {
        PHJ_TRY(np_limits(c, p));
        if (pairs) {
            PHJ_TRY(ensure(c, c->mat_mark, S.n * 4));   // a word per probe tuple, sized before the build
            PHJ_TRY(ensure(c, c->count, 32));
        }
        PHJ_TRY(np_setup(c, p, true, pay, J.np));
        if (pairs) PHJ_HIP(c, hipMemsetAsync(J.np.cnt, 0, 8, c->ks));
        J.hk = p->hash;
        J.seed = p->hash_seed;
        J.keys = !index ? 0 : S.columns ? 1 : 2;
        J.s_probe = J.keys == 1 ? reinterpret_cast<const longlong2*>(S.ckeys) : J.np.S_rel;
        J.nS = S.n;
        J.s_aos = index ? nullptr : J.np.S_rel;
        J.nF = static_cast<uint64_t>(J.np.g.nb) * kNPSlots;
        J.tab = J.np.tab;
        J.rp = J.np.pays;
        J.table_bytes = J.build_bytes = J.np.table_bytes;
        J.count_bytes = inner_count_bytes(0, S.n) + J.table_bytes;
        J.front_bytes = R.n * 32 + J.table_bytes;
        return PHJ_OK;
    }
    if (R.n >= (1ull << 32) - 1) return set_err(c, PHJ_ERR_RANGE, "build side above 2^32 tuples");
    if (S.n >= (1ull << 32) - 1) return set_err(c, PHJ_ERR_RANGE, "probe side above 2^32 tuples");
    PHJ_TRY(fused_setup(c, p, what, J.fu, pay));   // (pairs[] and the count words are its own workspace)
    J.hk = J.fu.pl.hk;
    J.nS = J.fu.nS;
    J.sk = S.view.keys;
    J.sp = S.view.payloads;
    J.nF = R.view.n;
    J.rk = R.view.keys;
    J.rp = R.view.payloads;
    J.build_bytes = R.n * 8;
    J.count_bytes = inner_count_bytes(R.n, J.nS);
    // (a key column's pass 1 reads 8 B per tuple less in each of its reads)
    J.front_bytes = partition_bytes(J.fu.pl, R.n) + partition_bytes(J.fu.pl, S.n) -
                    (index && R.columns ? R.n * 16 : 0) - (index && S.columns ? S.n * 16 : 0);
    J.num_partitions = J.fu.requested;
    return PHJ_OK;
}

// end: the event behind the join's last kernel.
int form_times(phj_ctx* c, const JoinForm& J, hipEvent_t end, phj_join_result* r) {
    return J.tab ? np_times(c, J.np.e0, J.np.e1, end, r) : fused_times(c, J.fu, end, r);
}

// k_np_inner / k_inner_fused over the form: the count pass (the radix form's
// work items before it), the count pass that also marks the build tuples it
// hits (the flags, c->row_hit, travel in its unused row pointer, phj_inner.h),
// and the emit pass of nrows rows into the sink in use.
enum class InnerPass { Count, CountMark, Emit };

int inner_pass(phj_ctx* c, const JoinForm& J, InnerPass pass, const RowSinks& out = {}, uint32_t nrows = 0) {
    auto* pairs = static_cast<uint32_t*>(c->mat_mark.p);
    JoinedRow* const flags = pass == InnerPass::CountMark ? static_cast<JoinedRow*>(c->row_hit.p) : nullptr;
    if (J.tab) {
        auto np = [&](auto h, auto keys, auto sink) {
            constexpr int HK = decltype(h)::value, KEYS = decltype(keys)::value;
            auto go = [&](auto kernel, auto to) {
                hipLaunchKernelGGL(kernel, dim3(J.np.grid), dim3(kBlock), 0, c->ks, J.s_probe, J.nS, J.tab, J.rp, J.np.g,
                                   J.seed, pairs, J.np.cnt, to, nrows);
            };
            if (pass == InnerPass::Emit) go(k_np_inner<HK, true, false, decltype(sink), KEYS>, sink);
            else if (pass == InnerPass::CountMark) go(k_np_inner<HK, false, true, JoinedRow*, KEYS>, flags);
            else go(k_np_inner<HK, false, false, JoinedRow*, KEYS>, flags);
        };
        with_hash(J.hk, [&](auto h) {   // (the index columns go with KEYS 1 or 2 and with nothing else)
            if (!J.index) np(h, std::integral_constant<int, 0>{}, out.rows);
            else if (J.keys == 1) np(h, std::integral_constant<int, 1>{}, out.index);
            else np(h, std::integral_constant<int, 2>{}, out.index);
        });
        PHJ_LAUNCHED(c, "k_np_inner");
        return PHJ_OK;
    }
    if (pass != InnerPass::Emit) PHJ_TRY(fused_work_items(c, J.fu));
    with_hash(J.hk, [&](auto h) {
        constexpr int HK = decltype(h)::value;
        auto go = [&](auto kernel, auto to) {
            hipLaunchKernelGGL(kernel, dim3(J.fu.grid), dim3(kBlock), 0, c->ks, J.fu.fa, pairs, J.sp, to, nrows);
        };
        if (pass == InnerPass::Emit)
            with_sink(J.index, out, [&](auto sink) { go(k_inner_fused<HK, true, false, decltype(sink)>, sink); });
        else if (pass == InnerPass::CountMark) go(k_inner_fused<HK, false, true>, flags);
        else go(k_inner_fused<HK, false>, flags);
    });
    PHJ_LAUNCHED(c, "k_inner_fused");
    return PHJ_OK;
}

// ---- aggregates over the join (phj_agg.h): totals and groups ----

// Bytes beyond partitioning / the table build (DESIGN.md §Aggregate joins).
// The totals pass reads both columns of both sides: 16 B per build tuple and
// 16 B per probe tuple (NoPartitioning: the table and a payload per build
// tuple instead of the build columns). Groups: per element of the build
// storage the 16-B accumulator cleared, updated and read, and 32 B per row.
uint64_t agg_join_bytes(uint64_t nR, uint64_t nS) { return nR * 16 + nS * 16; }
uint64_t agg_clear_bytes(uint64_t nF) { return nF * 16; }
uint64_t agg_compact_bytes(uint64_t nF, uint64_t rows) { return nF * 16 + rows * 32; }

// k_np_agg / k_agg_fused over the form (the radix form's work items before
// it): the totals into res and, with acc, the accumulator planes.
int agg_pass(phj_ctx* c, const JoinForm& J, unsigned long long* res, unsigned long long* acc) {
    if (!J.tab) PHJ_TRY(fused_work_items(c, J.fu));
    with_hash(J.hk, [&](auto h) {
        with_bool(acc != nullptr, [&](auto groups) {
            constexpr int HK = decltype(h)::value;
            constexpr bool GROUPS = decltype(groups)::value;
            if (J.tab)
                hipLaunchKernelGGL((k_np_agg<HK, GROUPS>), dim3(J.np.grid), dim3(kBlock), 0, c->ks, J.np.S_rel, J.nS, J.tab,
                                   J.rp, J.np.g, J.seed, res, acc, J.nF);
            else
                hipLaunchKernelGGL((k_agg_fused<HK, GROUPS>), dim3(J.fu.grid), dim3(kBlock), 0, c->ks, J.fu.fa, J.sp, res, acc,
                                   J.nF);
        });
    });
    PHJ_LAUNCHED(c, (J.tab ? "k_np_agg" : "k_agg_fused"));
    return PHJ_OK;
}

// Everything behind the partitioning / table build: the result words and
// (groups) the planes cleared, the accumulating pass, the compaction. One
// stream, one synchronisation at the end; *end: the event behind the last kernel.
int agg_passes(phj_ctx* c, uint32_t flags, const JoinForm& J, phj_join_result* r, phj_join_totals* t, hipEvent_t* end) {
    const bool groups = flags & PHJ_AGG_GROUPS, matched = flags & PHJ_AGG_MATCHED_ONLY;
    const uint64_t nR = c->side[PHJ_SIDE_BUILD].n;
    const uint32_t fblk = static_cast<uint32_t>((J.nF + kMatBlock - 1) / kMatBlock);
    PHJ_TRY(ensure(c, c->agg_res, 64));
    if (groups) {
        PHJ_TRY(ensure(c, c->agg_acc, J.nF * 16));
        PHJ_TRY(ensure(c, c->agg_cnt, (static_cast<size_t>(fblk) + 1) * 4));
        // (every build tuple may get a row; sized before the launch so that nothing is allocated between the passes)
        PHJ_TRY(ensure(c, c->agg_rows, std::max<uint64_t>(1, nR) * sizeof(GroupRow)));
    }
    auto* res = static_cast<unsigned long long*>(c->agg_res.p);   // {5 totals, group rows}
    auto* acc = static_cast<unsigned long long*>(c->agg_acc.p);
    auto* bcnt = static_cast<uint32_t*>(c->agg_cnt.p);
    PHJ_HIP(c, hipMemsetAsync(res, 0, 48, c->ks));
    if (groups) {
        const uint64_t bytes = agg_clear_bytes(J.nF);
        r->algorithmic_bytes += bytes;
        PHJ_TRY(timer_begin(c, "agg.groups", bytes));
        PHJ_HIP(c, hipMemsetAsync(acc, 0, J.nF * 16, c->ks));   // on every call: never the allocation's contents
        c->since_ev++;
        PHJ_TRY(timer_end(c));
    }
    const uint64_t jbytes = (J.tab ? agg_join_bytes(0, J.nS) + J.table_bytes + nR * 8 : agg_join_bytes(nR, J.nS)) +
                            (groups ? J.nF * 16 : 0);
    r->algorithmic_bytes += jbytes;
    PHJ_TRY(timer_begin(c, "agg.join", jbytes));
    PHJ_TRY(agg_pass(c, J, res, groups ? acc : nullptr));
    PHJ_TRY(timer_end(c));
    if (groups) {
        // (the rows written are only known afterwards: the timer carries the planes, the result adds the rows)
        PHJ_TRY(timer_begin(c, "agg.groups", agg_compact_bytes(J.nF, 0)));
        PHJ_HIP(c, hipMemsetAsync(bcnt, 0, (static_cast<size_t>(fblk) + 1) * 4, c->ks));
        auto* rows = static_cast<GroupRow*>(c->agg_rows.p);
        with_bool(J.tab != nullptr, [&](auto np) {
            hipLaunchKernelGGL(k_agg_group_count<decltype(np)::value>, dim3(fblk), dim3(kBlock), 0, c->ks, acc, J.tab, J.nF,
                               matched, bcnt, res + kAggTotals);
        });
        PHJ_LAUNCHED(c, "k_agg_group_count");
        PHJ_TRY(scan_u32(c, bcnt, fblk + 1, 1, fblk + 1));
        with_bool(J.tab != nullptr, [&](auto np) {
            hipLaunchKernelGGL(k_agg_group_write<decltype(np)::value>, dim3(fblk), dim3(kBlock), 0, c->ks, acc, J.tab, J.nF,
                               matched, J.rk, J.rp, bcnt, rows, nR);
        });
        PHJ_LAUNCHED(c, "k_agg_group_write");
        PHJ_TRY(timer_end(c));
    }
    PHJ_TRY(mark(c, end));
    unsigned long long h[kAggTotals + 1] = {0, 0, 0, 0, 0, 0};
    PHJ_HIP(c, hipMemcpyAsync(h, res, sizeof(h), hipMemcpyDeviceToHost, c->ks));
    PHJ_HIP(c, hipStreamSynchronize(c->ks));
    PHJ_TRY(check_chunk_errors(c));
    t->pairs = h[0];
    t->probe_matched = h[1];
    t->sum_a = static_cast<int64_t>(h[2]);
    t->sum_b = static_cast<int64_t>(h[3]);
    t->sum_ab = static_cast<int64_t>(h[4]);
    r->matches = t->pairs;
    if (groups) {
        if (h[kAggTotals] > nR) return set_err(c, PHJ_ERR_STATE, "phj_join_aggregate: more group rows than build tuples");
        c->agg_n = h[kAggTotals];
        r->algorithmic_bytes += agg_compact_bytes(J.nF, c->agg_n);
    }
    return PHJ_OK;
}

// An empty probe side with groups of every build tuple: rows copied from the
// bound relation, no join.
int agg_empty_probe(phj_ctx* c, phj_join_result* r) {
    const SideState& R = c->side[PHJ_SIDE_BUILD];
    PHJ_TRY(ensure(c, c->agg_rows, R.n * sizeof(GroupRow)));
    hipEvent_t e0, e1;
    PHJ_TRY(mark(c, &e0));
    PHJ_TRY(timer_begin(c, "agg.groups", R.n * (16 + 32)));
    const uint32_t grid = static_cast<uint32_t>(std::min<uint64_t>((R.n + kBlock - 1) / kBlock, 8192));
    hipLaunchKernelGGL(k_agg_group_side, dim3(grid), dim3(kBlock), 0, c->ks, reinterpret_cast<const longlong2*>(R.rel),
                       R.n, static_cast<GroupRow*>(c->agg_rows.p));
    PHJ_LAUNCHED(c, "k_agg_group_side");
    PHJ_TRY(timer_end(c));
    PHJ_TRY(mark(c, &e1));
    PHJ_HIP(c, hipStreamSynchronize(c->ks));
    c->agg_n = R.n;
    r->algorithmic_bytes = R.n * (16 + 32);
    r->probe_ms = r->total_ms = elapsed(c, e0, e1);
    return fill_timers(c, r);
}

// phj_join_aggregate.
int join_aggregate(phj_ctx* c, const phj_join_params* p, uint32_t flags, phj_join_result* r, phj_join_totals* t) {
    const char* what = "phj_join_aggregate";
    if (!c || !r || !t) return PHJ_ERR_INVALID;
    if (c->group) return set_err(c, PHJ_ERR_STATE, std::string(what) + ": single-device contexts only");
    if (!p) return set_err(c, PHJ_ERR_INVALID, "null params");
    if ((flags & ~static_cast<uint32_t>(PHJ_AGG_GROUPS | PHJ_AGG_MATCHED_ONLY)) ||
        ((flags & PHJ_AGG_MATCHED_ONLY) && !(flags & PHJ_AGG_GROUPS)))
        return set_err(c, PHJ_ERR_INVALID, std::string(what) + ": flags must be 0, PHJ_AGG_GROUPS or PHJ_AGG_GROUPS | PHJ_AGG_MATCHED_ONLY");
    PHJ_TRY(begin_call(c));
    std::memset(r, 0, sizeof(*r));
    std::memset(t, 0, sizeof(*t));
    c->agg_n = 0;
    if (p->algo != PHJ_ALGO_NO_PARTITIONING && p->algo != PHJ_ALGO_RADIX)
        return set_err(c, PHJ_ERR_INVALID, "Unrecognized join algorithm");
    PHJ_TRY(need_tuples_both(c, true, what));   // (sides bound as columns)
    const uint64_t nR = c->side[PHJ_SIDE_BUILD].n, nS = c->side[PHJ_SIDE_PROBE].n;
    // an empty side joins to nothing (no table to build, no pass to run)
    if (nR == 0 || nS == 0) {
        if (nR > 0 && flags == PHJ_AGG_GROUPS) PHJ_TRY(agg_empty_probe(c, r));
        return PHJ_OK;
    }
    JoinForm J;
    PHJ_TRY(form_setup(c, p, "radix aggregate join", false, false, J));   // (the totals land in agg_res)
    r->num_partitions = J.num_partitions;
    r->algorithmic_bytes = J.front_bytes;
    hipEvent_t end;
    PHJ_TRY(agg_passes(c, flags, J, r, t, &end));
    return form_times(c, J, end, r);
}

// ---- rows by class (phj_outer.h): pairs, probe-only, build-only ----

// What the passes of phj_join_rows must move beyond partitioning / the table
// build (DESIGN.md §Inner join, §Outer and anti joins). F = bytes of hit
// flags, one per element of the build storage. Count: the inner count pass;
// with build-only rows the flags cleared and (at most) every one stored; with
// probe-only rows pairs[] read and written and the bitmap written. Emit: the
// offsets (pairs[] read twice, written once); with the pair pass the build
// keys (or the table), the probe tuples and pairs[] read again and, per row, a
// build payload gathered and the row written; the bitmap read and, per null
// row, its offset, its probe tuple and the row written. Build-only: the flags
// read twice (count, write; NoPartitioning: with the table beside them) and,
// per row, a build tuple read and the row written.
uint64_t rows_count_bytes(uint64_t inner_count, uint64_t F, uint64_t nS, uint32_t classes) {
    return inner_count + ((classes & PHJ_ROWS_BUILD_ONLY) ? 2 * F : 0) +
           ((classes & PHJ_ROWS_PROBE_ONLY) ? nS * 8 + nS / 8 : 0);
}
// row: bytes written per row, 24 (phj_joined) or 16 (the two index columns).
uint64_t rows_emit_bytes(uint64_t nS, bool pair_pass, uint64_t pair_rows, uint64_t probe_only, uint64_t build_bytes,
                         uint64_t row) {
    return nS * 12 + (pair_pass ? build_bytes + nS * (16 + 4) + pair_rows * (8 + row) : 0) +
           (probe_only ? nS / 8 + probe_only * (4 + 16 + row) : 0);
}
uint64_t rows_build_only_bytes(uint64_t F, uint64_t table_bytes, uint64_t build_only, bool write, uint64_t row = 24) {
    return F + table_bytes + (write ? build_only * (16 + row) : 0);
}

// Where the row driver's two callers differ: phj_join_rows / phj_join_indices
// and phj_join_inner, which is their class PHJ_ROWS_PAIRS under older names.
struct RowsLabels {
    const char *count, *emit;   // the timers
    const char* radix;          // the radix form in its precondition message
    const char* unit;           // what the 2^32 message counts
    bool emit_always;           // the pair pass runs, and is accounted, with no pair to write
};
constexpr RowsLabels kRowsLabels{"rows.count", "rows.emit", "radix row join", "rows", false};
constexpr RowsLabels kInnerLabels{"inner.count", "inner.emit", "radix inner join", "pairs", true};

int rows_range_error(phj_ctx* c, const char* what, uint64_t rows, const char* unit = kRowsLabels.unit) {
    return set_err(c, PHJ_ERR_RANGE, std::string(what) + ": " + std::to_string(rows) + " " + unit +
                                         ", rows are addressed with 32 bits (limit 2^32 - 1)");
}

// Everything behind the partitioning / table build: the count pass (with hit
// marking) and the reductions, the counts read back, then (emit) the 2^32
// rule, offsets, pair rows, null rows and the unhit build tuples. One stream,
// one synchronisation at the end; *end: the event behind the last kernel.
int rows_passes(phj_ctx* c, uint32_t classes, int64_t null_payload, bool emit, const char* what, const RowsLabels& L,
                const JoinForm& J, phj_join_result* r, phj_row_counts* n, hipEvent_t* end) {
    const bool want_p = classes & PHJ_ROWS_PAIRS, want_s = classes & PHJ_ROWS_PROBE_ONLY,
               want_b = classes & PHJ_ROWS_BUILD_ONLY;
    const uint32_t nblk = static_cast<uint32_t>((J.nS + kMatBlock - 1) / kMatBlock);
    const uint32_t fblk = static_cast<uint32_t>((J.nF + kMatBlock - 1) / kMatBlock);
    if (want_s) PHJ_TRY(ensure(c, c->row_only, (J.nS + 63) / 64 * 8));
    if (want_b) {
        PHJ_TRY(ensure(c, c->row_hit, J.nF));
        PHJ_TRY(ensure(c, c->row_cnt, (static_cast<size_t>(fblk) + 1) * 4));
    }
    auto* pairs = static_cast<uint32_t*>(c->mat_mark.p);
    auto* cnt = static_cast<unsigned long long*>(c->count.p);   // {pairs, probe_only, build_only}
    auto* only = static_cast<uint64_t*>(c->row_only.p);
    auto* hit = static_cast<uint8_t*>(c->row_hit.p);
    auto* bcnt = static_cast<uint32_t*>(c->row_cnt.p);
    PHJ_HIP(c, hipMemsetAsync(cnt + 1, 0, 16, c->ks));
    uint64_t bytes = rows_count_bytes(J.count_bytes, J.nF, J.nS, classes);
    r->algorithmic_bytes += bytes;
    PHJ_TRY(timer_begin(c, L.count, bytes));
    if (want_b) PHJ_HIP(c, hipMemsetAsync(hit, 0, J.nF, c->ks));   // on every call: never the allocation's contents
    PHJ_TRY(inner_pass(c, J, want_b ? InnerPass::CountMark : InnerPass::Count));
    if (want_s) {
        with_bool(want_p, [&](auto wp) {
            hipLaunchKernelGGL(k_rows_map<decltype(wp)::value>, dim3(nblk), dim3(kBlock), 0, c->ks, pairs, J.nS, only, cnt + 1);
        });
        PHJ_LAUNCHED(c, "k_rows_map");
    }
    PHJ_TRY(timer_end(c));
    if (want_b) {
        bytes = rows_build_only_bytes(J.nF, J.table_bytes, 0, false);
        r->algorithmic_bytes += bytes;
        PHJ_TRY(timer_begin(c, "rows.build_only", bytes));
        PHJ_HIP(c, hipMemsetAsync(bcnt, 0, (static_cast<size_t>(fblk) + 1) * 4, c->ks));
        with_bool(J.tab != nullptr, [&](auto np) {
            hipLaunchKernelGGL(k_build_only_count<decltype(np)::value>, dim3(fblk), dim3(kBlock), 0, c->ks, hit, J.tab, J.nF,
                               bcnt, cnt + 2);
        });
        PHJ_LAUNCHED(c, "k_build_only_count");
        PHJ_TRY(timer_end(c));
    }
    PHJ_TRY(mark(c, end));
    unsigned long long h[3] = {0, 0, 0};
    PHJ_HIP(c, hipMemcpyAsync(h, cnt, sizeof(h), hipMemcpyDeviceToHost, c->ks));
    PHJ_HIP(c, hipStreamSynchronize(c->ks));
    PHJ_TRY(check_chunk_errors(c));
    n->pairs = h[0];
    n->probe_only = want_s ? h[1] : 0;
    n->build_only = want_b ? h[2] : 0;
    const uint64_t pair_rows = want_p ? n->pairs : 0;
    const uint64_t probe_rows = pair_rows + n->probe_only;
    n->rows = probe_rows + n->build_only;
    r->matches = n->rows;
    if (!emit) return PHJ_OK;
    // nothing is written and the row buffer is not grown above the limit
    // (below it no block sum of the offsets can have wrapped either)
    if (n->rows >= kInnerRowLimit) return rows_range_error(c, what, n->rows, L.unit);
    const uint64_t row_bytes = J.index ? 2 * sizeof(int64_t) : sizeof(JoinedRow);
    PHJ_TRY(ensure(c, c->mat_cnt, (static_cast<size_t>(nblk) + 1) * 4));
    PHJ_TRY(ensure(c, c->mat_rows, std::max<uint64_t>(1, n->rows) * row_bytes));
    const RowSinks out{static_cast<JoinedRow*>(c->mat_rows.p), index_sink(c, n->rows)};
    const bool pair_pass = pair_rows > 0 || L.emit_always;
    if (probe_rows > 0 || pair_pass) {
        bytes = rows_emit_bytes(J.nS, pair_pass, pair_rows, n->probe_only, J.build_bytes, row_bytes);
        r->algorithmic_bytes += bytes;
        PHJ_TRY(timer_begin(c, L.emit, bytes));
        PHJ_TRY(inner_offsets(c, J.nS));
        if (pair_pass) PHJ_TRY(inner_pass(c, J, InnerPass::Emit, out, static_cast<uint32_t>(probe_rows)));
        if (n->probe_only > 0) {
            const uint32_t grid = static_cast<uint32_t>(std::min<uint64_t>((J.nS + kBlock - 1) / kBlock, 8192));
            with_sink(J.index, out, [&](auto sink) {
                hipLaunchKernelGGL(k_rows_fill<decltype(sink)>, dim3(grid), dim3(kBlock), 0, c->ks, only, pairs, J.nS, J.s_aos,
                                   J.sk, J.sp, null_payload, sink, static_cast<uint32_t>(probe_rows));
            });
            PHJ_LAUNCHED(c, "k_rows_fill");
        }
        PHJ_TRY(timer_end(c));
    }
    if (n->build_only > 0) {
        bytes = rows_build_only_bytes(J.nF, J.table_bytes, n->build_only, true, row_bytes);
        r->algorithmic_bytes += bytes;
        PHJ_TRY(timer_begin(c, "rows.build_only", bytes));
        PHJ_TRY(scan_u32(c, bcnt, fblk + 1, 1, fblk + 1));
        const uint32_t row0 = static_cast<uint32_t>(probe_rows), nrows = static_cast<uint32_t>(n->rows);
        with_bool(J.tab != nullptr, [&](auto np) {
            with_sink(J.index, out, [&](auto sink) {
                hipLaunchKernelGGL((k_build_only_write<decltype(np)::value, decltype(sink)>), dim3(fblk), dim3(kBlock), 0, c->ks,
                                   hit, J.tab, J.nF, J.rk, J.rp, null_payload, bcnt, sink, row0, nrows);
            });
        });
        PHJ_LAUNCHED(c, "k_build_only_write");
        PHJ_TRY(timer_end(c));
    }
    PHJ_TRY(mark(c, end));
    PHJ_HIP(c, hipStreamSynchronize(c->ks));
    return PHJ_OK;
}

// An empty side: nothing to join; every tuple of the other side is "only".
int rows_empty_side(phj_ctx* c, uint32_t classes, int64_t null_payload, bool emit, const char* what, phj_join_result* r,
                    phj_row_counts* n, bool index) {
    const SideState& R = c->side[PHJ_SIDE_BUILD];
    const SideState& S = c->side[PHJ_SIDE_PROBE];
    n->probe_only = (classes & PHJ_ROWS_PROBE_ONLY) ? S.n : 0;   // (at least one of the two is empty)
    n->build_only = (classes & PHJ_ROWS_BUILD_ONLY) ? R.n : 0;
    n->rows = n->probe_only + n->build_only;
    r->matches = n->rows;
    if (!emit || n->rows == 0) return PHJ_OK;
    if (n->rows >= kInnerRowLimit) return rows_range_error(c, what, n->rows);
    const uint64_t row_bytes = index ? 2 * sizeof(int64_t) : sizeof(JoinedRow);
    PHJ_TRY(ensure(c, c->mat_rows, n->rows * row_bytes));
    const bool build = n->build_only > 0;
    const SideState& T = build ? R : S;
    hipEvent_t e0, e1;
    PHJ_TRY(mark(c, &e0));
    // (the index columns are written from the positions alone: nothing is read)
    const uint64_t bytes = n->rows * ((index ? 0 : 16) + row_bytes);
    PHJ_TRY(timer_begin(c, build ? "rows.build_only" : "rows.emit", bytes));
    const uint32_t grid = static_cast<uint32_t>(std::min<uint64_t>((T.n + kBlock - 1) / kBlock, 8192));
    const longlong2* rel = index ? nullptr : reinterpret_cast<const longlong2*>(T.rel);
    with_sink(index, RowSinks{static_cast<JoinedRow*>(c->mat_rows.p), index_sink(c, n->rows)}, [&](auto sink) {
        hipLaunchKernelGGL(k_rows_side<decltype(sink)>, dim3(grid), dim3(kBlock), 0, c->ks, rel, T.n, null_payload, build, sink);
    });
    PHJ_LAUNCHED(c, "k_rows_side");
    PHJ_TRY(timer_end(c));
    PHJ_TRY(mark(c, &e1));
    PHJ_HIP(c, hipStreamSynchronize(c->ks));
    r->algorithmic_bytes = bytes;
    r->probe_ms = r->total_ms = elapsed(c, e0, e1);
    return fill_timers(c, r);
}

// phj_join_rows_count (emit = false) / phj_join_rows, and with kInnerLabels
// and classes = PHJ_ROWS_PAIRS phj_join_inner_count / phj_join_inner.
// index: phj_join_indices (emit): keys only, no packed copy, the table's or
// the partitions' payloads are row numbers, the result in the two index columns.
int join_rows(phj_ctx* c, const phj_join_params* p, uint32_t classes, int64_t null_payload, phj_join_result* r,
              phj_row_counts* n, bool emit, const char* what, const RowsLabels& L = kRowsLabels, bool index = false) {
    if (!c || !r || !n) return PHJ_ERR_INVALID;
    if (c->group) return set_err(c, PHJ_ERR_STATE, std::string(what) + ": single-device contexts only");
    if (!p) return set_err(c, PHJ_ERR_INVALID, "null params");
    constexpr uint32_t all = PHJ_ROWS_PAIRS | PHJ_ROWS_PROBE_ONLY | PHJ_ROWS_BUILD_ONLY;
    if (classes == 0 || (classes & ~all))
        return set_err(c, PHJ_ERR_INVALID, std::string(what) + ": classes must be a non-empty set of PHJ_ROWS_*");
    PHJ_TRY(begin_call(c));
    std::memset(r, 0, sizeof(*r));
    std::memset(n, 0, sizeof(*n));
    if (emit) c->mat_n = c->idx_n = 0;   // one result at a time (the index columns lie in the row buffer)
    if (p->algo != PHJ_ALGO_NO_PARTITIONING && p->algo != PHJ_ALGO_RADIX)
        return set_err(c, PHJ_ERR_INVALID, "Unrecognized join algorithm");
    if (!index) PHJ_TRY(need_tuples_both(c, emit, what));   // (sides bound as columns)
    for (int side : {PHJ_SIDE_BUILD, PHJ_SIDE_PROBE})
        if (index && c->side[side].n > 0 && !c->side[side].rel && !c->side[side].columns)
            return set_err(c, PHJ_ERR_STATE, "relation not bound");
    // decided here: np_build refuses an empty build side, and no table or
    // partition is needed to know that the other side has no partner
    if (c->side[PHJ_SIDE_BUILD].n == 0 || c->side[PHJ_SIDE_PROBE].n == 0) {
        PHJ_TRY(rows_empty_side(c, classes, null_payload, emit, what, r, n, index));
    } else {
        JoinForm J;
        PHJ_TRY(form_setup(c, p, L.radix, true, index, J));
        r->num_partitions = J.num_partitions;
        r->algorithmic_bytes = J.front_bytes;
        hipEvent_t end;
        PHJ_TRY(rows_passes(c, classes, null_payload, emit, what, L, J, r, n, &end));
        PHJ_TRY(form_times(c, J, end, r));
    }
    if (emit) (index ? c->idx_n : c->mat_n) = n->rows;
    return PHJ_OK;
}


int ctx_create_device(int device, phj_ctx** out) {
    if (!out) return PHJ_ERR_INVALID;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return PHJ_ERR_HIP;
    if (device < 0 || device >= ndev) return PHJ_ERR_INVALID;
    if (hipSetDevice(device) != hipSuccess) return PHJ_ERR_HIP;
    phj_ctx* c = new phj_ctx();
    c->device = device;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return PHJ_ERR_HIP;
    }
    if (hipStreamCreateWithFlags(&c->aux, hipStreamNonBlocking) != hipSuccess) {
        (void)hipStreamDestroy(c->stream);
        delete c;
        return PHJ_ERR_HIP;
    }
    c->ks = c->stream;
    c->own_stream = true;
    {
        const int t = env_int("PHJ_TILE", 4096);
        c->tune.tile = (t == 2048 || t == 8192) ? t : 4096;
    }
    c->tune.block = env_int("PHJ_BLOCK", 512);
    c->tune.nt_load = std::min(2, std::max(0, env_int("PHJ_NT_LOAD", 1)));
    c->tune.fused = env_int("PHJ_FUSED", 1) != 0;
    c->tune.ptab = env_int("PHJ_PTAB", 1);
    c->tune.subpart = env_int("PHJ_SUBPART", 1) != 0;
    c->tune.timers = env_int("PHJ_TIMERS", 1) != 0;
    c->tune.p1_chunk = env_int("PHJ_P1_CHUNK", 1) != 0;
    c->tune.cluster = env_int("PHJ_CLUSTER", 1) != 0;
    c->tune.p1_pipe = env_int("PHJ_P1_PIPE", 1) != 0;
    c->tune.cl_cap = env_int("PHJ_CL_CAP", static_cast<int>(kClCapMax)) == 8192 ? 8192 : static_cast<int>(kClCapMax);
    c->tune.cl_bits = std::max(0, std::min(kMaxDigitBits, env_int("PHJ_CL_BITS", 0)));
    c->tune.p2probe = env_int("PHJ_P2PROBE", 1);
    c->tune.p1_slots = env_int("PHJ_P1_SLOTS", 0);
    c->tune.p1_wpc2 = std::max(0, env_int("PHJ_P1_WPC2", 2));
    c->tune.r_order = std::min(2, std::max(0, env_int("PHJ_R_ORDER", 1)));
    c->tune.count_pin = env_int("PHJ_COUNT_PIN", 1);
    c->tune.r_chunk = env_int("PHJ_R_CHUNK", 1) != 0;
    c->tune.p1_block = env_int("PHJ_P1_BLOCK", 1024) == 512 ? 512 : 1024;
    c->tune.p1_tps = std::max(1, env_int("PHJ_P1_TPS", static_cast<int>(kTilesPerShard)));
    c->tune.p1_min_tiles = std::max(0, env_int("PHJ_P1_MIN_TILES", 32768));
    c->tune.p1_ko_tps = std::max(1, env_int("PHJ_P1_KO_TPS", 1024));
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess) c->num_cus = prop.multiProcessorCount;
    }
    // gfx950 launches accept dynamic LDS up to the 160 KiB per workgroup without an
    // opt-in attribute; clear any error a probe of the runtime left behind
    (void)hipGetLastError();
    *out = c;
    return PHJ_OK;
}

}  // namespace

#include "phj_group.h"

namespace {

// A multi-device context with one local member forwards the single-device
// calls (building blocks) to it; with several members they are not defined.
template <class F>
int on_solo(phj_ctx* c, const char* what, F f) {
    phj_ctx* m = c->group->nlocal() == 1 ? c->group->mem[0] : nullptr;
    if (!m) return set_err(c, PHJ_ERR_STATE, std::string(what) + ": not available on a multi-device context");
    const int rc = f(m);
    if (rc != PHJ_OK) c->err = m->err;
    return rc;
}

// ---- phj_join's three radix paths (radix_path), each from the plan it runs ----
// requested: the partitions asked for, as the result reports them.

// PHJ_PATH_LDS_JOIN (phj_cluster.h). cpl: the cluster plan.
int join_lds(phj_ctx* c, const Plan& cpl, uint32_t requested, phj_join_result* r) {
    SideState& R = c->side[PHJ_SIDE_BUILD];
    SideState& S = c->side[PHJ_SIDE_PROBE];
    hipEvent_t t0, t1, tr, b0, p1;
    // a side bound as columns: its code pass reads the key column where it
    // has the column form (cols_native), else the side is packed first
    const bool s_cols = cols_native(c, S, cpl, false), r_cols = cols_native(c, R, cpl, true);
    if (!r_cols) PHJ_TRY(need_tuples(c, PHJ_SIDE_BUILD, false, "phj_join"));
    if (!s_cols) PHJ_TRY(need_tuples(c, PHJ_SIDE_PROBE, false, "phj_join"));
    // the LDS join (phj_cluster.h): S's pass 1 into clusters (codes) on
    // the main stream; R's pass 1 and the big clusters' HBM tables on the
    // aux stream beside it; then the probe builds each cluster's table in
    // LDS and probes S's codes against it
    PHJ_TRY(ensure(c, c->count, 32));
    // the result's phase marks: with deferred timers nothing reads them
    // (the result's phase times stay zero) and, R's chain on the main
    // stream, no stream waits on them: not recorded (each event between
    // two kernels delays the second by ~4 us)
    const int order = c->tune.r_order;
    const bool r_main = order == 1;
    const bool no_marks = c->defer_timers && r_main;
    t0 = tr = b0 = t1 = p1 = nullptr;
    auto phase_mark = [&](hipEvent_t* e) -> int { return no_marks ? PHJ_OK : mark_shared(c, e); };
    if (!no_marks) PHJ_TRY(mark(c, &t0));
    const int64_t* rcodes = nullptr;
    const uint32_t* rbnd = nullptr;
    // R's chain on the aux stream, after event `after`
    // R in tile mode (PHJ_R_CHUNK, default): R through the chunked code
    // pass as S (one launch; 8 shards, so a cluster below the LDS limit
    // has at most 8 + 3 runs), its tiles read by the builds; else the
    // stable pass (k_hist + scan + k_scatter_codes: codes contiguous per cluster)
    SideState* RT = nullptr;
    // after S's pass (PHJ_R_ORDER=1, default) R's chain runs on the main
    // stream itself: nothing runs beside it, and a cross-stream event wait
    // before the probe costs ~15 us (measured gap, r05z timeline)
    // with the hot-key pre-aggregation (phj_hot.h): R's
    // chain on the aux stream from the join's start, beside the hot-key
    // prologue (a few narrow kernels bound by atomics), its pass 1 leaving
    // the prologue PHJ_HOT_FREE_CUS CUs per shard; the main stream waits
    // for it before the LDS join. R's chain reads nothing of S's: the
    // weights are resolved by the LDS join, not by R's pass
    const bool hot = hot_wanted(c, cpl, S.n, R.n);
    const bool early_r = hot && R.n > 0;
    auto r_chain = [&](hipEvent_t after) -> int {
        if (!r_main || early_r) {
            PHJ_HIP(c, hipStreamWaitEvent(c->aux, after, 0));
            c->ks = c->aux;
        }
        int rc = PHJ_OK;
        if (c->tune.r_chunk && R.n > 0) {
            c->p1_free_cus = early_r ? PHJ_HOT_FREE_CUS : 0;
            rc = partition_state(c, R, "R", cpl, true, nullptr, 8);
            c->p1_free_cus = 0;
            if (rc == PHJ_OK && R.hcoded) RT = &R;
        }
        if (!RT) {
            if (rc == PHJ_OK) rc = ensure(c, c->r_codes, std::max<uint64_t>(1, R.n) * 8);
            if (rc == PHJ_OK) rc = ensure(c, c->r_bounds, (static_cast<size_t>(cpl.nb1) + 1) * 4);
            rcodes = static_cast<const int64_t*>(c->r_codes.p);
            rbnd = static_cast<const uint32_t*>(c->r_bounds.p);
            if (rc == PHJ_OK) rc = partition_build(c, cpl, static_cast<int64_t*>(c->r_codes.p), static_cast<uint32_t*>(c->r_bounds.p));
        }
        if (rc == PHJ_OK) rc = phase_mark(&b0);
        // the HBM tables of clusters beyond the LDS limit (none at the
        // balanced configurations; the LDS tables are built inside the probe)
        if (rc == PHJ_OK) rc = timer_begin(c, "build.big", 0);
        if (rc == PHJ_OK) rc = cluster_big_fill(c, cpl, 1, &rcodes, &rbnd, R.n, RT);
        if (rc == PHJ_OK) rc = timer_end(c);
        if (rc == PHJ_OK) rc = phase_mark(&tr);
        c->ks = c->stream;
        return rc;
    };
    // PHJ_R_ORDER: 0 = R's chain beside S's pass 1 (it waits for t0: the
    // previous step's probe read R's codes), 1 = after S's pass 1, 2 = before it
    if (order == 2) {
        PHJ_TRY(r_chain(t0));
        PHJ_HIP(c, hipStreamWaitEvent(c->stream, tr, 0));
    }
    // the code pass's bookkeeping kernel clears the count pair (an empty
    // S takes no chunked pass: a memset). R's chain after S's pass on the
    // same stream: S's bookkeeping kernel also clears R's chunk state (one
    // memset launch and its gap fewer before R's pass; not with R's chain
    // ahead of S's pass: its state is in use by then, cleared by a memset
    // on the aux stream ahead of R's pass)
    const bool pre_clear = r_main && !early_r && c->tune.r_chunk && R.n > 0 && !c->dry;
    if (pre_clear) {
        PHJ_TRY(ensure(c, R.ccur, chunk_state_bytes(cpl.nb1)));
        c->p1_clear = R.ccur.p;
        c->p1_clear_bytes = chunk_state_bytes(cpl.nb1);
    }
    if (early_r) {
        // the fork, before the prologue: the previous join's probe
        // read R's pool and tile list
        for (hipEvent_t* e : {&c->hot_fork, &c->hot_join})
            if (!*e && !(*e = new_event())) return set_err(c, PHJ_ERR_HIP, "hipEventCreate failed");
        PHJ_HIP(c, hipEventRecord(c->hot_fork, c->stream));
    }
    // hot probe keys (phj_hot.h): sampled and selected here; S's pass then
    // counts them instead of writing them, the LDS join looks them up in
    // the tables it builds and adds the weights of those R holds to the
    // count (after S's bookkeeping kernel has cleared it: one stream)
    struct HotScope {
        phj_ctx* c;
        bool ok = false;   // the join ran to its end (else the hot state is cleared before its next use)
        ~HotScope() {
            c->hot_on = false;
            if (!ok) c->hot_clean = nullptr;
        }
    } hot_scope{c};
    if (hot) PHJ_TRY(hot_begin(c, cpl, S));
    if (early_r) {
        // issued after the prologue's launches (the main stream is the
        // step's critical path: each launch is a few us of host time) and
        // ahead of S's pass, which is not held back by it: the workgroups
        // of S's pass whose CUs R still holds start when R's pass ends
        int rc = r_chain(c->hot_fork);
        if (rc == PHJ_OK && hipEventRecord(c->hot_join, c->aux) != hipSuccess) rc = set_err(c, PHJ_ERR_HIP, "hipEventRecord failed");
        PHJ_TRY(rc);
    }
    const int prc = partition_side(c, PHJ_SIDE_PROBE, cpl, true, static_cast<unsigned long long*>(c->count.p));
    c->p1_clear = nullptr;
    if (prc != PHJ_OK) {
        c->p1_cleared = nullptr;
        return prc;
    }
    if (!S.hcoded) PHJ_HIP(c, hipMemsetAsync(c->count.p, 0, 32, c->stream));
    if (order != 2 && !early_r) {
        const int rc = r_chain(t0);
        c->p1_cleared = nullptr;   // (R's pass may not have taken the chunked form)
        PHJ_TRY(rc);
    }
    if (!r_main) PHJ_HIP(c, hipStreamWaitEvent(c->stream, tr, 0));
    if (early_r) PHJ_HIP(c, hipStreamWaitEvent(c->stream, c->hot_join, 0));
    if (c->hot_on && R.n > 0 && !RT) return set_err(c, PHJ_ERR_STATE, "hot-key pre-aggregation needs R's chunked code pass");
    PHJ_TRY(phase_mark(&t1));
    // one launch, reported as "build" (the workgroups' table builds in LDS:
    // R's codes read) and "probe" (S's codes read), split by the kernel's own clocks
    PHJ_TRY(timer_begin_split(c, R.n * 8, S.n * 8));
    if (c->lean_timers && c->tune.timers) {   // build.big not timed: a zero-length record keeps the phase listed
        const hipEvent_t e = c->timers.back().a;
        c->timers.insert(c->timers.end() - 2, TimerRec{"build.big", 0, e, e});
    }
    c->count_pinned = false;
    PHJ_TRY(probe_cluster(c, cpl, S, 1, &rcodes, &rbnd, RT, true));
    PHJ_TRY(timer_end_split(c));
    PHJ_TRY(phase_mark(&p1));
    uint64_t m = 0;
    PHJ_TRY(get_count(c, &m, true));
    r->matches = m;
    r->partition_ms = elapsed(c, t0, t1);
    {   // the probe launch split by its clocks (build = the LDS table builds + the big clusters' HBM tables)
        const double t = elapsed(c, t1, p1), fb = c->tune.timers && !c->defer_timers ? fused_build_fraction(c) : 0.0;
        r->build_ms = elapsed(c, b0, tr) + t * fb;
        r->probe_ms = t * (1.0 - fb);
    }
    r->total_ms = elapsed(c, t0, p1);
    r->num_partitions = requested;
    // R: 16 read + 8 written (pass 1), 8 read (probe); S: 16 read + 8 written, 8 read
    // (a key column: 8 read in pass 1)
    r->algorithmic_bytes = R.n * (24 + 8) + S.n * (24 + 8) - (r_cols ? R.n * 8 : 0) - (s_cols ? S.n * 8 : 0);
    hot_scope.ok = true;
    return fill_timers(c, r);
}

// PHJ_PATH_CODE_TABLES (phj_table.h). pl: the refined plan.
int join_code_tables(phj_ctx* c, const Plan& pl, uint32_t requested, phj_join_result* r) {
    SideState& R = c->side[PHJ_SIDE_BUILD];
    SideState& S = c->side[PHJ_SIDE_PROBE];
    hipEvent_t t0, t1, tr, b0, p1;
    PHJ_TRY(need_tuples_both(c, false, "phj_join"));   // (sides bound as columns: no column form on this path)
    // S: pass 1 only (its pass 2 runs inside the probe); R: pass 1 as codes
    // and its tables on the aux stream, beside S (measured: R's chain
    // issued first, or run before S with S's pass 1 on every LDS slot, is
    // 0.05-0.1 ms slower; probing S in row ranges, each beside the next
    // range's pass 1, is 0.3 ms slower: DESIGN.md section 3)
    PHJ_TRY(ensure(c, c->count, 32));
    PHJ_TRY(mark(c, &t0));
    // the code pass's bookkeeping kernel clears the count (hcoded)
    PHJ_TRY(partition_side(c, PHJ_SIDE_PROBE, pl, true, static_cast<unsigned long long*>(c->count.p)));
    // R's chain waits for t0 (the previous step's probe read its tables);
    // the wait is issued after S's pass 1 so that launch goes out first
    PHJ_HIP(c, hipStreamWaitEvent(c->aux, t0, 0));
    c->ks = c->aux;
    int rc = ensure(c, c->r_codes, std::max<uint64_t>(1, R.n) * 8);
    if (rc == PHJ_OK) rc = ensure(c, c->r_bounds, (static_cast<size_t>(pl.Ppad) + 1) * 4);
    const int64_t* rcodes = static_cast<const int64_t*>(c->r_codes.p);
    const uint32_t* rbnd = static_cast<const uint32_t*>(c->r_bounds.p);
    if (rc == PHJ_OK) rc = partition_build(c, pl, static_cast<int64_t*>(c->r_codes.p), static_cast<uint32_t*>(c->r_bounds.p));
    if (rc == PHJ_OK) rc = mark(c, &b0);
    // algorithmic bytes: the codes read, the tables written (~1.7 slots per code)
    if (rc == PHJ_OK) rc = timer_begin(c, "build", R.n * 8 * 3);
    if (rc == PHJ_OK) rc = build_ht(c, pl, 1, &rcodes, &rbnd, R.n);
    if (rc == PHJ_OK) rc = timer_end(c);
    if (rc == PHJ_OK) rc = mark(c, &tr);
    c->ks = c->stream;
    PHJ_TRY(rc);
    PHJ_HIP(c, hipStreamWaitEvent(c->stream, tr, 0));
    PHJ_TRY(mark(c, &t1));
    // algorithmic bytes: the pass-1 output read once (16-B tuples, or 8-B
    // codes after a keys-only pass 1); the tables are re-read from L2
    PHJ_TRY(timer_begin(c, "probe", S.n * (S.p2.keys_only ? 8 : 16)));
    PHJ_TRY(probe_ht(c, pl, S, !S.hcoded));
    PHJ_TRY(timer_end(c));
    PHJ_TRY(mark(c, &p1));
    uint64_t m = 0;
    PHJ_TRY(get_count(c, &m, true));
    r->matches = m;
    r->partition_ms = elapsed(c, t0, t1);
    r->build_ms = elapsed(c, b0, tr);
    r->probe_ms = elapsed(c, t1, p1);
    r->total_ms = elapsed(c, t0, p1);
    r->num_partitions = requested;
    r->algorithmic_bytes = R.n * (24 + 16) + S.n * (16 + 8) + R.n * 24 + S.n * 8;
    return fill_timers(c, r);
}

// PHJ_PATH_PARTITIONED: both sides fully partitioned, then build_and_probe. pl: the refined plan.
int join_partitioned_sides(phj_ctx* c, const Plan& pl, uint32_t requested, phj_join_result* r) {
    SideState& R = c->side[PHJ_SIDE_BUILD];
    SideState& S = c->side[PHJ_SIDE_PROBE];
    hipEvent_t t0, t1, tr, b0, b1, p1;
    PHJ_TRY(need_tuples_both(c, false, "phj_join"));   // (sides bound as columns: no column form on this path)
    // Partition(R) || Partition(S) (HashJoin.hpp:210-216): S (the long one) is
    // issued first on the ctx stream, R beside it on the aux stream
    PHJ_TRY(mark(c, &t0));
    PHJ_HIP(c, hipStreamWaitEvent(c->aux, t0, 0));
    PHJ_TRY(partition_side(c, PHJ_SIDE_PROBE, pl));
    c->ks = c->aux;
    int rc = partition_side(c, PHJ_SIDE_BUILD, pl);
    if (rc == PHJ_OK) rc = mark(c, &tr);
    c->ks = c->stream;
    PHJ_TRY(rc);
    PHJ_HIP(c, hipStreamWaitEvent(c->stream, tr, 0));
    PHJ_TRY(mark(c, &t1));
    PHJ_TRY(build_and_probe(c, pl, 1, &R.view, &b0, &b1, &p1));
    uint64_t m = 0;
    PHJ_TRY(get_count(c, &m));
    r->matches = m;
    r->partition_ms = elapsed(c, t0, t1);
    r->build_ms = elapsed(c, b0, b1);
    r->probe_ms = elapsed(c, b1, p1);
    if (c->last_fused) {   // one fused launch: split by the kernel's own build / probe clocks
        const double t = elapsed(c, b0, p1), fb = fused_build_fraction(c);
        r->build_ms = t * fb;
        r->probe_ms = t * (1.0 - fb);
    }
    r->total_ms = elapsed(c, t0, p1);
    r->num_partitions = requested;
    r->algorithmic_bytes = partition_bytes(pl, R.n) + partition_bytes(pl, S.n) + R.n * 32 + S.n * 8 + R.n * 8;
    return fill_timers(c, r);
}

}  // namespace

extern "C" {

int phj_abi_version(void) { return PHJ_ABI_VERSION; }

int phj_ctx_create_device(int device, phj_ctx** out) { return ctx_create_device(device, out); }

int phj_ctx_create_ex(int ngpus, const int* devs, uint32_t flags, phj_ctx** out) {
    if (!out) return PHJ_ERR_INVALID;
    *out = nullptr;
    if (ngpus < 1 || ngpus > kMaxSegs) return PHJ_ERR_INVALID;
    std::vector<int> d(ngpus);
    for (int i = 0; i < ngpus; i++) d[i] = devs ? devs[i] : i;
    if (ngpus == 1 && !(flags & (PHJ_CTX_EXCHANGE | PHJ_CTX_LOCAL))) return ctx_create_device(d[0], out);
    return group_create(ngpus, d.data(), flags, ngpus, 0, nullptr, out);
}

int phj_ctx_create(int ngpus, const int* devs, phj_ctx** out) { return phj_ctx_create_ex(ngpus, devs, 0, out); }

int phj_comm_unique_id(uint8_t* id) {
    if (!id) return PHJ_ERR_INVALID;
    RcclApi& api = rccl();
    if (!api.loaded) {
        std::fprintf(stderr, "phj_comm_unique_id: %s\n", api.err.c_str());
        return PHJ_ERR_HIP;
    }
    static_assert(sizeof(ncclUniqueId) == PHJ_UNIQUE_ID_BYTES, "unique id size");
    ncclUniqueId u;
    if (api.GetUniqueId(&u) != ncclSuccess) return PHJ_ERR_HIP;
    std::memcpy(id, &u, sizeof(u));
    return PHJ_OK;
}

int phj_ctx_create_rank(int device, int nranks, int rank, const uint8_t* id, phj_ctx** out) {
    if (!out) return PHJ_ERR_INVALID;
    *out = nullptr;
    if (!id || nranks < 1 || nranks > kMaxSegs || rank < 0 || rank >= nranks) return PHJ_ERR_INVALID;
    return group_create(1, &device, 0, nranks, rank, id, out);
}

int phj_ctx_info(const phj_ctx* c, int* world, int* rank0, int* nlocal) {
    if (!c) return PHJ_ERR_INVALID;
    if (world) *world = c->group ? c->group->world : 1;
    if (rank0) *rank0 = c->group ? c->group->rank0 : 0;
    if (nlocal) *nlocal = c->group ? c->group->nlocal() : 1;
    return PHJ_OK;
}

void phj_shard_range(uint64_t n, int rank, int world, uint64_t* lo, uint64_t* hi) {
    uint64_t a = 0, b = 0;
    if (world >= 1 && rank >= 0 && rank < world) shard_range(n, rank, world, &a, &b);
    if (lo) *lo = a;
    if (hi) *hi = b;
}

void phj_exchange_layout(uint64_t max_shard, uint32_t num_partitions, uint64_t* codes_elems, uint64_t* block_elems) {
    const uint64_t cap = (max_shard + 63) / 64 * 64;   // both columns stay 16-B aligned in the gathered buffer
    if (codes_elems) *codes_elems = cap;
    if (block_elems) *block_elems = cap + (static_cast<uint64_t>(num_partitions) + 2) / 2;
}

int phj_join_path(const phj_join_params* p, uint64_t build_n, uint64_t probe_n) {
    if (!p) return PHJ_ERR_INVALID;
    if (p->algo == PHJ_ALGO_NO_PARTITIONING) return PHJ_PATH_NO_PARTITIONING;
    if (p->algo != PHJ_ALGO_RADIX) return PHJ_ERR_INVALID;
    phj_ctx tmp;   // default tuning (no device is touched)
    Plan pl, run;
    if (make_plan(&tmp, p, pl) != PHJ_OK) return PHJ_ERR_INVALID;
    return radix_path(&tmp, pl, probe_n, build_n, run);
}

int phj_exchange_geometry(const phj_join_params* p, uint64_t total_build, uint32_t* num_segments, uint32_t* shift,
                          uint32_t* sub_bits, uint32_t* sub_shift, int* cluster) {
    if (!p || p->algo != PHJ_ALGO_RADIX) return PHJ_ERR_INVALID;
    phj_ctx tmp;   // default tuning (no device is touched)
    Plan pl, cpl;
    if (make_plan(&tmp, p, pl) != PHJ_OK) return PHJ_ERR_INVALID;
    const bool cl = use_cluster(&tmp, pl, 0, total_build, cpl);
    if (cl) pl = cpl;
    else refine_plan(&tmp, pl, total_build);
    if (num_segments) *num_segments = cl ? pl.nb1 : pl.Ppad;
    if (shift) *shift = cl ? pl.shift1 : 0;
    if (sub_bits) *sub_bits = pl.sub_bits;
    if (sub_shift) *sub_shift = pl.sub_shift;
    if (cluster) *cluster = cl ? 1 : 0;
    return PHJ_OK;
}

void phj_count_contribution(uint64_t count, int failed, uint64_t* words) {
    words[0] = failed ? 0 : count;
    words[1] = failed ? 1 : 0;
}

int phj_count_verdict(const uint64_t* words, uint64_t* matches) {
    if (words[1] != 0) return PHJ_ERR_STATE;
    if (matches) *matches = words[0];
    return PHJ_OK;
}

void phj_ctx_destroy(phj_ctx* c) {
    if (!c) return;
    if (c->group) {
        group_destroy(c->group);
        delete c;
        return;
    }
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    (void)hipStreamSynchronize(c->aux);
    if (c->count_host) (void)hipHostFree(c->count_host);
    if (c->count_pin) (void)hipHostFree(c->count_pin);
    for (SideState& S : c->side) {
        for (DevBuf* b : {&S.owned, &S.ck, &S.cp, &S.pack, &S.kA, &S.pA, &S.kB, &S.pB, &S.hist1, &S.hist2, &S.bounds1, &S.tbase2,
                          &S.bounds, &S.partials, &S.tseg2, &S.dig, &S.ccur, &S.ctab, &S.tstart, &S.csink})
            free_buf(*b);
    }
    for (DevBuf* b : {&c->ht_tab, &c->ht_desc, &c->r_codes, &c->r_bounds, &c->scan_partials, &c->prep, &c->tkeys, &c->tpays, &c->toffs, &c->gcursor, &c->items, &c->biglist,
                      &c->count, &c->np_tab, &c->np_pays, &c->np_ovf, &c->np_ovfb, &c->np_ovfn, &c->fitems, &c->split, &c->cl_prof, &c->mat_mark, &c->mat_cnt, &c->mat_rows, &c->row_hit, &c->row_only, &c->row_cnt, &c->agg_acc, &c->agg_cnt, &c->agg_rows, &c->agg_res, &c->cl_done, &c->hot, &c->gather_bad, &c->member_marks})
        free_buf(*b);
    for (phj_index* ix : c->indexes) {
        if (ix->tab) (void)hipFree(ix->tab);
        if (ix->first_rows) (void)hipFree(ix->first_rows);
        delete ix;
    }
    for (hipEvent_t e : c->evpool) (void)hipEventDestroy(e);
    for (hipEvent_t e : {c->hot_fork, c->hot_join})
        if (e) (void)hipEventDestroy(e);
    if (c->own_stream) (void)hipStreamDestroy(c->stream);
    (void)hipStreamDestroy(c->aux);
    delete c;
}

const char* phj_last_error(const phj_ctx* c) { return c ? c->err.c_str() : "null context"; }

int phj_ctx_set_stream(phj_ctx* c, void* stream) {
    if (!c) return PHJ_ERR_INVALID;
    if (c->group) return on_solo(c, "phj_ctx_set_stream", [&](phj_ctx* m) { return phj_ctx_set_stream(m, stream); });
    PHJ_HIP(c, hipSetDevice(c->device));
    PHJ_HIP(c, hipStreamSynchronize(c->stream));
    PHJ_HIP(c, hipStreamSynchronize(c->aux));
    if (c->own_stream) {
        PHJ_HIP(c, hipStreamDestroy(c->stream));
        c->own_stream = false;
    }
    if (stream) {
        c->stream = static_cast<hipStream_t>(stream);
    } else {
        PHJ_HIP(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        c->own_stream = true;
    }
    c->ks = c->stream;
    return PHJ_OK;
}

int phj_ctx_synchronize(phj_ctx* c) {
    if (!c) return PHJ_ERR_INVALID;
    if (c->group) {
        for (phj_ctx* m : c->group->mem) {
            const int rc = phj_ctx_synchronize(m);
            if (rc != PHJ_OK) return set_err(c, rc, m->err);
        }
        return PHJ_OK;
    }
    PHJ_HIP(c, hipStreamSynchronize(c->aux));
    PHJ_HIP(c, hipStreamSynchronize(c->stream));
    return PHJ_OK;
}

int phj_relation_upload(phj_ctx* c, int side, const phj_tuple* host, uint64_t n) {
    PHJ_TRY(check_side(c, side));
    if (n && !host) return set_err(c, PHJ_ERR_INVALID, "null host relation");
    if (c->group) return group_upload(c, side, host, n);
    PHJ_HIP(c, hipSetDevice(c->device));
    SideState& S = c->side[side];
    drop_relation(c, side);
    PHJ_TRY(ensure(c, S.owned, n * sizeof(phj_tuple)));
    if (n) {
        PHJ_HIP(c, hipMemcpyAsync(S.owned.p, host, n * sizeof(phj_tuple), hipMemcpyHostToDevice, c->ks));
        PHJ_HIP(c, hipStreamSynchronize(c->ks));
    }
    S.rel = static_cast<const phj_tuple*>(S.owned.p);
    S.n = n;
    return PHJ_OK;
}

int phj_relation_bind_device(phj_ctx* c, int side, const phj_tuple* dev, uint64_t n) {
    PHJ_TRY(check_side(c, side));
    if (n && !dev) return set_err(c, PHJ_ERR_INVALID, "null device relation");
    if (reinterpret_cast<uintptr_t>(dev) % 16) return set_err(c, PHJ_ERR_INVALID, "relation must be 16-byte aligned");
    if (c->group) {
        PHJ_TRY(on_solo(c, "phj_relation_bind_device", [&](phj_ctx* m) { return phj_relation_bind_device(m, side, dev, n); }));
        return exchange_sizes(c, *c->group, side);
    }
    drop_relation(c, side);
    c->side[side].rel = dev;
    c->side[side].n = n;
    return PHJ_OK;
}

const phj_tuple* phj_relation_device_ptr(phj_ctx* c, int side, uint64_t* n) {
    if (!c || (side != 0 && side != 1)) return nullptr;
    if (c->group) {   // several local devices: rows of all of them, no single pointer
        if (c->group->nlocal() == 1) return phj_relation_device_ptr(c->group->mem[0], side, n);
        if (n) {
            *n = 0;
            for (phj_ctx* m : c->group->mem) *n += m->side[side].n;
        }
        return nullptr;
    }
    if (n) *n = c->side[side].n;
    if (c->side[side].columns) return nullptr;   // (phj_relation_columns serves a columnar binding)
    return c->side[side].rel;
}

int phj_relation_download(phj_ctx* c, int side, phj_tuple* host, uint64_t n) {
    PHJ_TRY(check_side(c, side));
    if (c->group) return group_download(c, side, host, n);
    SideState& S = c->side[side];
    if (n > S.n) return set_err(c, PHJ_ERR_INVALID, "download larger than the relation");
    PHJ_HIP(c, hipSetDevice(c->device));
    if (n && S.columns && !S.packed) {   // the columns copied back and interleaved on the host (payload 0 without a payload column)
        if (!host) return set_err(c, PHJ_ERR_INVALID, "null destination");
        std::vector<int64_t> col;
        try {
            col.resize(n);
        } catch (const std::exception&) {
            return set_err(c, PHJ_ERR_NOMEM, "no host memory to stage a column of " + std::to_string(n) + " keys");
        }
        for (int f = 0; f < 2; f++) {
            const int64_t* src = f == 0 ? S.ckeys : S.cpays;
            if (src) {
                PHJ_HIP(c, hipMemcpyAsync(col.data(), src, n * 8, hipMemcpyDeviceToHost, c->ks));
                PHJ_HIP(c, hipStreamSynchronize(c->ks));
            }
            for (uint64_t i = 0; i < n; i++) (f == 0 ? host[i].id : host[i].payload) = src ? col[i] : 0;
        }
        return PHJ_OK;
    }
    if (n) {
        PHJ_HIP(c, hipMemcpyAsync(host, S.rel, n * sizeof(phj_tuple), hipMemcpyDeviceToHost, c->ks));
        PHJ_HIP(c, hipStreamSynchronize(c->ks));
    }
    return PHJ_OK;
}

// ---- relations bound as columns ----
static_assert(sizeof(phj_relation_info) == 24, "phj_relation_info layout");

// The side's binding replaced by the columns k / p (p null: keys alone).
static void bind_columns_state(phj_ctx* c, int side, const int64_t* k, const int64_t* p, uint64_t n, bool owned) {
    drop_relation(c, side);
    SideState& S = c->side[side];
    S.columns = true;
    S.cols_owned = owned;
    S.ckeys = k;
    S.cpays = p;
    S.n = n;
    c->hot_clean = nullptr;   // the next hot-key prologue starts from cleared counters
}

static int columns_guard(phj_ctx* c, int side, const char* what) {
    PHJ_TRY(check_side(c, side));
    if (c->group) return set_err(c, PHJ_ERR_STATE, std::string(what) + ": single-device contexts only");
    return PHJ_OK;
}

int phj_relation_upload_columns(phj_ctx* c, int side, const int64_t* keys, const int64_t* payloads, uint64_t n) {
    PHJ_TRY(columns_guard(c, side, "phj_relation_upload_columns"));
    if (n && !keys) return set_err(c, PHJ_ERR_INVALID, "null host key column");
    PHJ_HIP(c, hipSetDevice(c->device));
    SideState& S = c->side[side];
    drop_relation(c, side);
    PHJ_TRY(ensure(c, S.ck, n * 8));
    if (payloads) PHJ_TRY(ensure(c, S.cp, n * 8));
    if (n) {
        PHJ_HIP(c, hipMemcpyAsync(S.ck.p, keys, n * 8, hipMemcpyHostToDevice, c->ks));
        if (payloads) PHJ_HIP(c, hipMemcpyAsync(S.cp.p, payloads, n * 8, hipMemcpyHostToDevice, c->ks));
        PHJ_HIP(c, hipStreamSynchronize(c->ks));
    }
    bind_columns_state(c, side, static_cast<const int64_t*>(S.ck.p), payloads ? static_cast<const int64_t*>(S.cp.p) : nullptr, n, true);
    return PHJ_OK;
}

int phj_relation_bind_columns(phj_ctx* c, int side, const int64_t* dev_keys, const int64_t* dev_payloads, uint64_t n) {
    PHJ_TRY(columns_guard(c, side, "phj_relation_bind_columns"));
    if (n && !dev_keys) return set_err(c, PHJ_ERR_INVALID, "null device key column");
    if (reinterpret_cast<uintptr_t>(dev_keys) % 8 || reinterpret_cast<uintptr_t>(dev_payloads) % 8)
        return set_err(c, PHJ_ERR_INVALID, "columns must be 8-byte aligned");
    bind_columns_state(c, side, dev_keys, dev_payloads, n, false);
    return PHJ_OK;
}

int phj_relation_to_columns(phj_ctx* c, int side, int with_payloads) {
    PHJ_TRY(columns_guard(c, side, "phj_relation_to_columns"));
    SideState& S = c->side[side];
    if (S.columns) {   // already columns: only the payload column may go, and with it a packed copy that holds it
        if (!with_payloads && S.cpays) {
            S.cpays = nullptr;
            S.packed = false;
            S.rel = nullptr;
            S.partitioned = false;
        }
        return PHJ_OK;
    }
    if (!S.rel && S.n > 0) return set_err(c, PHJ_ERR_STATE, "relation not bound");
    PHJ_HIP(c, hipSetDevice(c->device));
    const uint64_t n = S.n;
    PHJ_TRY(ensure(c, S.ck, n * 8));
    if (with_payloads) PHJ_TRY(ensure(c, S.cp, n * 8));
    if (n) {
        const uint32_t g = static_cast<uint32_t>(std::min<uint64_t>((n + kBlock - 1) / kBlock, 65536));
        hipLaunchKernelGGL(k_split_columns, dim3(g), dim3(kBlock), 0, c->ks, reinterpret_cast<const longlong2*>(S.rel), n,
                           static_cast<int64_t*>(S.ck.p), with_payloads ? static_cast<int64_t*>(S.cp.p) : nullptr);
        PHJ_LAUNCHED(c, "k_split_columns");
        PHJ_HIP(c, hipStreamSynchronize(c->ks));
    }
    bind_columns_state(c, side, static_cast<const int64_t*>(S.ck.p), with_payloads ? static_cast<const int64_t*>(S.cp.p) : nullptr, n, true);
    return PHJ_OK;
}

int phj_relation_columns(phj_ctx* c, int side, const int64_t** keys, const int64_t** payloads, uint64_t* n) {
    PHJ_TRY(columns_guard(c, side, "phj_relation_columns"));
    const SideState& S = c->side[side];
    if (keys) *keys = S.columns ? S.ckeys : nullptr;
    if (payloads) *payloads = S.columns ? S.cpays : nullptr;
    if (n) *n = S.n;
    return PHJ_OK;
}

int phj_relation_info_get(phj_ctx* c, int side, phj_relation_info* out) {
    PHJ_TRY(columns_guard(c, side, "phj_relation_info_get"));
    if (!out) return set_err(c, PHJ_ERR_INVALID, "null destination");
    const SideState& S = c->side[side];
    out->n = S.n;
    out->layout = S.columns ? PHJ_LAYOUT_COLUMNS : PHJ_LAYOUT_TUPLES;
    out->has_payloads = !S.columns || S.cpays ? 1u : 0u;
    out->packed = S.columns && S.packed ? 1u : 0u;
    out->owned = S.columns ? (S.cols_owned ? 1u : 0u) : (S.rel && S.rel == S.owned.p ? 1u : 0u);
    return PHJ_OK;
}

int phj_relation_generate_sequential(phj_ctx* c, int side, uint64_t n, int64_t start, uint64_t first_index) {
    PHJ_TRY(check_side(c, side));
    if (c->group)
        return group_generate(c, side, n, first_index, [&](phj_ctx* m, uint64_t k, uint64_t first) {
            return phj_relation_generate_sequential(m, side, k, start, first);
        });
    PHJ_HIP(c, hipSetDevice(c->device));
    SideState& S = c->side[side];
    drop_relation(c, side);
    PHJ_TRY(ensure(c, S.owned, n * sizeof(phj_tuple)));
    if (n) {
        const uint32_t g = static_cast<uint32_t>(std::min<uint64_t>((n + kBlock - 1) / kBlock, 65536));
        hipLaunchKernelGGL(k_gen_sequential, dim3(g), dim3(kBlock), 0, c->ks, static_cast<longlong2*>(S.owned.p), n, start,
                           first_index);
        PHJ_LAUNCHED(c, "k_gen_sequential");
        PHJ_HIP(c, hipStreamSynchronize(c->ks));
    }
    S.rel = static_cast<const phj_tuple*>(S.owned.p);
    S.n = n;
    return PHJ_OK;
}

int phj_relation_generate_zipf(phj_ctx* c, int side, uint64_t n, double alpha, int64_t lo, int64_t hi,
                               uint64_t seed, uint64_t first_index) {
    PHJ_TRY(check_side(c, side));
    if (lo >= hi) return set_err(c, PHJ_ERR_INVALID, "Range for Zipf generation is incorrectly specified");
    if (alpha < 0.01) return set_err(c, PHJ_ERR_INVALID, "Skew parameter must be greater than 0.01.");
    if (c->group)
        return group_generate(c, side, n, first_index, [&](phj_ctx* m, uint64_t k, uint64_t first) {
            return phj_relation_generate_zipf(m, side, k, alpha, lo, hi, seed, first);
        });
    PHJ_HIP(c, hipSetDevice(c->device));
    SideState& S = c->side[side];
    drop_relation(c, side);
    PHJ_TRY(ensure(c, S.owned, n * sizeof(phj_tuple)));
    if (n) {
        const uint64_t b0 = first_index / kGenBatch, b1 = (first_index + n + kGenBatch - 1) / kGenBatch;
        const uint32_t g = static_cast<uint32_t>((b1 - b0 + kBlock - 1) / kBlock);
        hipLaunchKernelGGL(k_gen_zipf, dim3(g), dim3(kBlock), 0, c->ks, static_cast<longlong2*>(S.owned.p), n,
                           alpha, static_cast<uint64_t>(hi - lo + 1), lo - 1, seed, first_index);
        PHJ_LAUNCHED(c, "k_gen_zipf");
        PHJ_HIP(c, hipStreamSynchronize(c->ks));
    }
    S.rel = static_cast<const phj_tuple*>(S.owned.p);
    S.n = n;
    return PHJ_OK;
}

int phj_relation_count_in_range(phj_ctx* c, int side, int64_t lo, int64_t hi, uint64_t* count) {
    PHJ_TRY(check_side(c, side));
    if (!count) return set_err(c, PHJ_ERR_INVALID, "null count");
    if (c->group) {   // over this process's shards
        uint64_t t = 0;
        for (phj_ctx* m : c->group->mem) {
            uint64_t k = 0;
            const int rc = phj_relation_count_in_range(m, side, lo, hi, &k);
            if (rc != PHJ_OK) return set_err(c, rc, m->err);
            t += k;
        }
        *count = t;
        return PHJ_OK;
    }
    PHJ_TRY(begin_call(c, 0, true));   // (it records no timer and leaves those of earlier calls)
    SideState& S = c->side[side];
    PHJ_TRY(ensure(c, c->count, 8));
    PHJ_HIP(c, hipMemsetAsync(c->count.p, 0, 8, c->ks));
    if (S.n && S.columns) {   // over the key column itself
        const uint32_t g = static_cast<uint32_t>(std::min<uint64_t>((S.n + kBlock - 1) / kBlock, 8192));
        hipLaunchKernelGGL(k_count_range_col, dim3(g), dim3(kBlock), 0, c->ks, S.ckeys, S.n, lo, hi,
                           static_cast<unsigned long long*>(c->count.p));
        PHJ_LAUNCHED(c, "k_count_range_col");
    } else if (S.n) {
        const uint32_t g = static_cast<uint32_t>(std::min<uint64_t>((S.n + kBlock - 1) / kBlock, 8192));
        hipLaunchKernelGGL(k_count_range, dim3(g), dim3(kBlock), 0, c->ks, reinterpret_cast<const longlong2*>(S.rel),
                           S.n, lo, hi, static_cast<unsigned long long*>(c->count.p));
        PHJ_LAUNCHED(c, "k_count_range");
    }
    return get_count(c, count);
}

int phj_partition(phj_ctx* c, int side, const phj_join_params* p, phj_partitioned* out) {
    PHJ_TRY(check_side(c, side));
    if (c->group) return on_solo(c, "phj_partition", [&](phj_ctx* m) { return phj_partition(m, side, p, out); });
    if (p && p->algo != PHJ_ALGO_RADIX) return set_err(c, PHJ_ERR_INVALID, "phj_partition needs PHJ_ALGO_RADIX");
    Plan pl;
    PHJ_TRY(make_plan(c, p, pl));
    // timers accumulate until phj_join / phj_join_partitioned / phj_timers_report reports them
    PHJ_TRY(begin_call(c, 0, true));
    PHJ_TRY(need_tuples(c, side, false, "phj_partition"));   // (bound as columns: the payloads of a key column alone are 0)
    PHJ_TRY(partition_side(c, side, pl));
    if (out) *out = c->side[side].view;
    return PHJ_OK;
}

int phj_join_partitioned(phj_ctx* c, const phj_join_params* p, int nbuild, const phj_partitioned* build,
                         phj_join_result* r) {
    if (!c || !r) return PHJ_ERR_INVALID;
    if (c->group)
        return on_solo(c, "phj_join_partitioned", [&](phj_ctx* m) { return phj_join_partitioned(m, p, nbuild, build, r); });
    if (!build) return set_err(c, PHJ_ERR_INVALID, "null build segments");
    if (p && p->algo != PHJ_ALGO_RADIX) return set_err(c, PHJ_ERR_INVALID, "phj_join_partitioned needs PHJ_ALGO_RADIX");
    Plan pl;
    PHJ_TRY(make_plan(c, p, pl));
    PHJ_TRY(begin_call(c, 0, true));   // (with the phj_partition timers since the last report)
    std::memset(r, 0, sizeof(*r));
    hipEvent_t b0, b1, p1;
    PHJ_TRY(build_and_probe(c, pl, nbuild, build, &b0, &b1, &p1));
    uint64_t m = 0;
    PHJ_TRY(get_count(c, &m));
    r->matches = m;
    r->build_ms = elapsed(c, b0, b1);
    r->probe_ms = elapsed(c, b1, p1);
    if (c->last_fused) {   // one fused launch: split by the kernel's own build / probe clocks
        const double t = elapsed(c, b0, p1), fb = fused_build_fraction(c);
        r->build_ms = t * fb;
        r->probe_ms = t * (1.0 - fb);
    }
    r->total_ms = elapsed(c, b0, p1);
    r->num_partitions = pl.Ppad;
    uint64_t nR = 0;
    for (int g = 0; g < nbuild; g++) nR += build[g].n;
    r->algorithmic_bytes = nR * 32 + c->side[PHJ_SIDE_PROBE].view.n * 8 + nR * 8;
    const int rc = fill_timers(c, r);  // includes the phj_partition launches since the last report
    reset_timers(c);
    return rc;
}

int phj_join_partitioned_async(phj_ctx* c, const phj_join_params* p, int nbuild, const phj_partitioned* build,
                               uint64_t* dev_count) {
    if (!c) return PHJ_ERR_INVALID;
    if (c->group)
        return on_solo(c, "phj_join_partitioned_async",
                       [&](phj_ctx* m) { return phj_join_partitioned_async(m, p, nbuild, build, dev_count); });
    if (!build || !dev_count) return set_err(c, PHJ_ERR_INVALID, "null build segments or count address");
    if (p && p->algo != PHJ_ALGO_RADIX)
        return set_err(c, PHJ_ERR_INVALID, "phj_join_partitioned_async needs PHJ_ALGO_RADIX");
    Plan pl;
    PHJ_TRY(make_plan(c, p, pl));
    PHJ_TRY(begin_call(c, 0, true));
    hipEvent_t b0, b1, p1;
    PHJ_TRY(build_and_probe(c, pl, nbuild, build, &b0, &b1, &p1));
    PHJ_HIP(c, hipMemcpyAsync(dev_count, c->count.p, 8, hipMemcpyDeviceToDevice, c->ks));
    return PHJ_OK;
}

int phj_join(phj_ctx* c, const phj_join_params* p, phj_join_result* r) {
    if (!c || !r) return PHJ_ERR_INVALID;
    if (!p) return set_err(c, PHJ_ERR_INVALID, "null params");
    if (c->group) {
        (void)hipGetLastError();   // (the members' calls have no prologue of their own)
        std::memset(r, 0, sizeof(*r));
        return group_join(c, p, r, false);
    }
    PHJ_TRY(begin_call(c, p->flags));   // (PHJ_DEFER_TIMERS: its timers stay for phj_timers_report)
    std::memset(r, 0, sizeof(*r));
    c->hot_ran = false;
    if (p->algo == PHJ_ALGO_NO_PARTITIONING) {
        PHJ_TRY(need_tuples_both(c, false, "phj_join"));   // (sides bound as columns)
        return join_nopart(c, p, r);
    }
    if (p->algo != PHJ_ALGO_RADIX) return set_err(c, PHJ_ERR_INVALID, "Unrecognized join algorithm");
    Plan pl, run;
    PHJ_TRY(make_plan(c, p, pl));
    const uint32_t requested = pl.Ppad;   // reported; the join may sub-partition
    switch (radix_path(c, pl, c->side[PHJ_SIDE_PROBE].n, c->side[PHJ_SIDE_BUILD].n, run)) {
        case PHJ_PATH_LDS_JOIN: return join_lds(c, run, requested, r);
        case PHJ_PATH_CODE_TABLES: return join_code_tables(c, run, requested, r);
        default: return join_partitioned_sides(c, run, requested, r);
    }
}

int phj_prepare(phj_ctx* c, const phj_join_params* p) {
    if (!c) return PHJ_ERR_INVALID;
    if (!p) return set_err(c, PHJ_ERR_INVALID, "null params");
    if (c->group) {
        phj_join_result r{};
        return group_join(c, p, &r, true);
    }
    PHJ_TRY(begin_call(c, 0, true));   // (no timer is recorded; those of earlier calls stay)
    PHJ_TRY(reserve_events(c, kPrepEvents));
    struct DryScope {
        phj_ctx* c;
        ~DryScope() { c->dry = false; }
    } scope{c};
    c->dry = true;
    if (p->algo == PHJ_ALGO_NO_PARTITIONING) {
        phj_join_result r{};
        PHJ_TRY(need_tuples_both(c, false, "phj_prepare"));
        return join_nopart(c, p, &r);
    }
    if (p->algo != PHJ_ALGO_RADIX) return set_err(c, PHJ_ERR_INVALID, "Unrecognized join algorithm");
    Plan asked, pl;
    PHJ_TRY(make_plan(c, p, asked));
    const uint64_t nR = c->side[PHJ_SIDE_BUILD].n;
    // the workspace of the path phj_join takes (radix_path), by that path's own
    // sizing calls; its bodies (join_lds ...) record events, wait across streams
    // and read the count back, so they are listed here, not run dry
    const int path = radix_path(c, asked, c->side[PHJ_SIDE_PROBE].n, nR, pl);
    if (path == PHJ_PATH_LDS_JOIN) {
        const Plan& cpl = pl;
        // (sides bound as columns: the tuple copy of a side phj_join would pack)
        if (!cols_native(c, c->side[PHJ_SIDE_BUILD], cpl, true)) PHJ_TRY(need_tuples(c, PHJ_SIDE_BUILD, false, "phj_prepare"));
        if (!cols_native(c, c->side[PHJ_SIDE_PROBE], cpl, false)) PHJ_TRY(need_tuples(c, PHJ_SIDE_PROBE, false, "phj_prepare"));
        if (PHJ_PREAGG) PHJ_TRY(ensure(c, c->hot, hot_state_bytes(cpl.nb1)));
        PHJ_TRY(partition_side(c, PHJ_SIDE_PROBE, cpl, true));
        PHJ_TRY(ensure(c, c->r_codes, std::max<uint64_t>(1, nR) * 8));
        PHJ_TRY(ensure(c, c->r_bounds, (static_cast<size_t>(cpl.nb1) + 1) * 4));
        PHJ_TRY(partition_build(c, cpl, nullptr, nullptr));
        PHJ_TRY(cluster_big_fill(c, cpl, 1, nullptr, nullptr, nR));
        PHJ_HIP(c, hipStreamSynchronize(c->stream));
        return PHJ_OK;
    }
    PHJ_TRY(need_tuples_both(c, false, "phj_prepare"));
    if (path == PHJ_PATH_CODE_TABLES) {
        PHJ_TRY(partition_side(c, PHJ_SIDE_PROBE, pl, true));
        PHJ_TRY(ensure(c, c->r_codes, std::max<uint64_t>(1, nR) * 8));
        PHJ_TRY(ensure(c, c->r_bounds, (static_cast<size_t>(pl.Ppad) + 1) * 4));
        PHJ_TRY(partition_build(c, pl, nullptr, nullptr));
        PHJ_TRY(build_ht(c, pl, 1, nullptr, nullptr, nR));
        PHJ_TRY(ensure(c, c->count, 32));
        PHJ_HIP(c, hipStreamSynchronize(c->stream));
        return PHJ_OK;
    }
    PHJ_TRY(partition_side(c, PHJ_SIDE_PROBE, pl));
    PHJ_TRY(partition_side(c, PHJ_SIDE_BUILD, pl));
    phj_partitioned seg{};
    seg.n = c->side[PHJ_SIDE_BUILD].n;
    seg.num_partitions = pl.Ppad;
    hipEvent_t b0, b1, p1;
    PHJ_TRY(build_and_probe(c, pl, 1, &seg, &b0, &b1, &p1));
    PHJ_HIP(c, hipStreamSynchronize(c->stream));
    return PHJ_OK;
}

int phj_timers_report(phj_ctx* c, phj_join_result* r) {
    if (!c || !r) return PHJ_ERR_INVALID;
    if (c->group) return on_solo(c, "phj_timers_report", [&](phj_ctx* m) { return phj_timers_report(m, r); });
    PHJ_HIP(c, hipSetDevice(c->device));
    PHJ_HIP(c, hipStreamSynchronize(c->ks));
    std::memset(r, 0, sizeof(*r));
    c->defer_timers = false;
    c->lean_timers = false;
    const int rc = fill_timers(c, r);
    reset_timers(c);
    return rc;
}

int phj_partitioned_download(phj_ctx* c, const phj_partitioned* v, int64_t* keys, int64_t* payloads,
                             uint32_t* bounds) {
    if (!c || !v) return PHJ_ERR_INVALID;
    if (c->group)
        return on_solo(c, "phj_partitioned_download",
                       [&](phj_ctx* m) { return phj_partitioned_download(m, v, keys, payloads, bounds); });
    PHJ_HIP(c, hipSetDevice(c->device));
    if (v->n && keys) PHJ_HIP(c, hipMemcpyAsync(keys, v->keys, v->n * 8, hipMemcpyDefault, c->ks));
    if (v->n && payloads) PHJ_HIP(c, hipMemcpyAsync(payloads, v->payloads, v->n * 8, hipMemcpyDefault, c->ks));
    if (bounds)
        PHJ_HIP(c, hipMemcpyAsync(bounds, v->bounds, (static_cast<size_t>(v->num_partitions) + 1) * 4,
                                  hipMemcpyDefault, c->ks));
    // device-only destinations stay stream-ordered; host destinations need the wait
    auto on_device = [](const void* ptr) {
        if (!ptr) return true;
        hipPointerAttribute_t at{};
        if (hipPointerGetAttributes(&at, ptr) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        return at.type == hipMemoryTypeDevice;
    };
    if (!(on_device(keys) && on_device(payloads) && on_device(bounds))) {
        PHJ_HIP(c, hipStreamSynchronize(c->ks));
        PHJ_TRY(check_chunk_errors(c));   // a chunked pass that met a stale table wrote nothing through it
    }
    return PHJ_OK;
}

static_assert(sizeof(phj_joined) == 24 && sizeof(JoinedRow) == sizeof(phj_joined), "JoinedTuple layout");

int phj_join_materialize(phj_ctx* c, const phj_join_params* p, phj_join_result* r) {
    if (!c || !r) return PHJ_ERR_INVALID;
    if (c->group) return set_err(c, PHJ_ERR_STATE, "phj_join_materialize: single-device contexts only");
    if (!p) return set_err(c, PHJ_ERR_INVALID, "null params");
    PHJ_TRY(begin_call(c));
    std::memset(r, 0, sizeof(*r));
    c->mat_n = c->idx_n = 0;   // (the index columns of phj_join_indices lie in the same buffer)
    PHJ_TRY(need_tuples_both(c, true, "phj_join_materialize"));   // (sides bound as columns)
    if (p->algo == PHJ_ALGO_NO_PARTITIONING) {
        SideState& S = c->side[PHJ_SIDE_PROBE];
        if (S.n >= (1ull << 32)) return set_err(c, PHJ_ERR_RANGE, "probe side above 2^32 tuples");
        PHJ_TRY(ensure(c, c->mat_mark, std::max<uint64_t>(1, S.n) * 4));
        PHJ_TRY(join_nopart(c, p, r, static_cast<uint32_t*>(c->mat_mark.p)));
        hipEvent_t e0, e1;
        PHJ_TRY(mark(c, &e0));
        PHJ_TRY(mat_compact(c, S.n, reinterpret_cast<const longlong2*>(S.rel), nullptr, nullptr,
                            static_cast<const int64_t*>(c->np_pays.p)));
        PHJ_TRY(mark(c, &e1));
        PHJ_HIP(c, hipStreamSynchronize(c->ks));
        r->probe_ms += elapsed(c, e0, e1);
        r->total_ms += elapsed(c, e0, e1);
        r->algorithmic_bytes += r->matches * 24;
        PHJ_TRY(fill_timers(c, r));
    } else if (p->algo == PHJ_ALGO_RADIX) {
        PHJ_TRY(join_radix_mark(c, p, r));
    } else {
        return set_err(c, PHJ_ERR_INVALID, "Unrecognized join algorithm");
    }
    c->mat_n = r->matches;
    return PHJ_OK;
}

int phj_join_inner_count(phj_ctx* c, const phj_join_params* p, phj_join_result* r) {
    phj_row_counts n;
    return join_rows(c, p, PHJ_ROWS_PAIRS, 0, r, &n, false, "phj_join_inner_count", kInnerLabels);
}

int phj_join_inner(phj_ctx* c, const phj_join_params* p, phj_join_result* r) {
    phj_row_counts n;
    return join_rows(c, p, PHJ_ROWS_PAIRS, 0, r, &n, true, "phj_join_inner", kInnerLabels);
}

int phj_join_rows_count(phj_ctx* c, const phj_join_params* p, uint32_t classes, phj_join_result* r,
                        phj_row_counts* n) {
    return join_rows(c, p, classes, 0, r, n, false, "phj_join_rows_count");
}

int phj_join_rows(phj_ctx* c, const phj_join_params* p, uint32_t classes, int64_t null_payload, phj_join_result* r,
                  phj_row_counts* n) {
    return join_rows(c, p, classes, null_payload, r, n, true, "phj_join_rows");
}

const phj_joined* phj_joined_rows(phj_ctx* c, uint64_t* n) {
    if (!c || c->group) return nullptr;
    if (n) *n = c->mat_n;
    return static_cast<const phj_joined*>(c->mat_rows.p);
}

int phj_joined_download(phj_ctx* c, phj_joined* host, uint64_t n) {
    if (!c) return PHJ_ERR_INVALID;
    if (c->group) return set_err(c, PHJ_ERR_STATE, "phj_joined_download: single-device contexts only");
    if (n > c->mat_n) return set_err(c, PHJ_ERR_RANGE, "more rows requested than the last materialised join made");
    if (n == 0) return PHJ_OK;
    if (!host) return set_err(c, PHJ_ERR_INVALID, "null destination");
    PHJ_HIP(c, hipSetDevice(c->device));
    PHJ_HIP(c, hipMemcpyAsync(host, c->mat_rows.p, n * sizeof(phj_joined), hipMemcpyDeviceToHost, c->stream));
    PHJ_HIP(c, hipStreamSynchronize(c->stream));
    return PHJ_OK;
}

// ---- row-number joins (phj_index.h) ----

int phj_join_indices(phj_ctx* c, const phj_join_params* p, uint32_t classes, phj_join_result* r, phj_row_counts* n) {
    return join_rows(c, p, classes, PHJ_NO_ROW, r, n, true, "phj_join_indices", kRowsLabels, true);
}

int phj_joined_indices(phj_ctx* c, const int64_t** build_rows, const int64_t** probe_rows, uint64_t* n) {
    if (!c) return PHJ_ERR_INVALID;
    if (c->group) return set_err(c, PHJ_ERR_STATE, "phj_joined_indices: single-device contexts only");
    const IndexSink s = index_sink(c, c->idx_n);
    if (build_rows) *build_rows = c->idx_n ? s.build_rows : nullptr;
    if (probe_rows) *probe_rows = c->idx_n ? s.probe_rows : nullptr;
    if (n) *n = c->idx_n;
    return PHJ_OK;
}

int phj_joined_indices_download(phj_ctx* c, int64_t* build_rows, int64_t* probe_rows, uint64_t n) {
    if (!c) return PHJ_ERR_INVALID;
    if (c->group) return set_err(c, PHJ_ERR_STATE, "phj_joined_indices_download: single-device contexts only");
    if (n > c->idx_n) return set_err(c, PHJ_ERR_RANGE, "more rows requested than the last index join made");
    if (n == 0) return PHJ_OK;
    PHJ_HIP(c, hipSetDevice(c->device));
    const IndexSink s = index_sink(c, c->idx_n);
    // (hipMemcpyDefault: the destinations may be host or device memory)
    if (build_rows) PHJ_HIP(c, hipMemcpyAsync(build_rows, s.build_rows, n * 8, hipMemcpyDefault, c->stream));
    if (probe_rows) PHJ_HIP(c, hipMemcpyAsync(probe_rows, s.probe_rows, n * 8, hipMemcpyDefault, c->stream));
    PHJ_HIP(c, hipStreamSynchronize(c->stream));
    return PHJ_OK;
}

int phj_gather_column(phj_ctx* c, const int64_t* src, uint64_t src_n, const int64_t* idx, uint64_t n,
                      const int64_t* null_value, int64_t* out) {
    if (!c) return PHJ_ERR_INVALID;
    if (c->group) return set_err(c, PHJ_ERR_STATE, "phj_gather_column: single-device contexts only");
    (void)hipGetLastError();
    if (n == 0) return PHJ_OK;
    if (!idx || !out || (src_n && !src)) return set_err(c, PHJ_ERR_INVALID, "null argument");
    if ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(idx) | reinterpret_cast<uintptr_t>(out)) & 7)
        return set_err(c, PHJ_ERR_INVALID, "phj_gather_column: columns need 8-byte alignment");
    if (src_n >= (1ull << 63)) return set_err(c, PHJ_ERR_RANGE, "phj_gather_column: src_n above 2^63");
    PHJ_HIP(c, hipSetDevice(c->device));
    PHJ_TRY(ensure(c, c->gather_bad, 8));
    auto* bad = static_cast<unsigned long long*>(c->gather_bad.p);
    PHJ_HIP(c, hipMemsetAsync(bad, 0, 8, c->stream));
    const uint32_t grid = static_cast<uint32_t>(std::min<uint64_t>((n + kBlock - 1) / kBlock, static_cast<uint64_t>(c->num_cus) * 32));
    if (null_value)
        hipLaunchKernelGGL(k_gather_column<false>, dim3(grid), dim3(kBlock), 0, c->stream, src, src_n, idx, n, *null_value, out, bad);
    else
        hipLaunchKernelGGL(k_gather_column<true>, dim3(grid), dim3(kBlock), 0, c->stream, src, src_n, idx, n, int64_t{0}, out, bad);
    PHJ_LAUNCHED(c, "k_gather_column");
    unsigned long long h = 0;
    PHJ_HIP(c, hipMemcpyAsync(&h, bad, 8, hipMemcpyDeviceToHost, c->stream));
    PHJ_HIP(c, hipStreamSynchronize(c->stream));
    if (h)
        return set_err(c, PHJ_ERR_RANGE, "phj_gather_column: " + std::to_string(h) + " indices outside [0, " +
                                             std::to_string(src_n) + ") other than PHJ_NO_ROW: not dereferenced, given the null treatment");
    return PHJ_OK;
}

int phj_join_aggregate(phj_ctx* c, const phj_join_params* p, uint32_t flags, phj_join_result* r, phj_join_totals* t) {
    return join_aggregate(c, p, flags, r, t);
}

const phj_group_row* phj_group_rows(phj_ctx* c, uint64_t* n) {
    if (!c || c->group) return nullptr;
    if (n) *n = c->agg_n;
    return static_cast<const phj_group_row*>(c->agg_rows.p);
}

int phj_group_download(phj_ctx* c, phj_group_row* host, uint64_t n) {
    if (!c) return PHJ_ERR_INVALID;
    if (c->group) return set_err(c, PHJ_ERR_STATE, "phj_group_download: single-device contexts only");
    if (n > c->agg_n) return set_err(c, PHJ_ERR_RANGE, "more rows requested than the last aggregate join made");
    if (n == 0) return PHJ_OK;
    if (!host) return set_err(c, PHJ_ERR_INVALID, "null destination");
    PHJ_HIP(c, hipSetDevice(c->device));
    PHJ_HIP(c, hipMemcpyAsync(host, c->agg_rows.p, n * sizeof(phj_group_row), hipMemcpyDeviceToHost, c->stream));
    PHJ_HIP(c, hipStreamSynchronize(c->stream));
    return PHJ_OK;
}

// ---- membership joins (phj_member.h) ----
static_assert(sizeof(phj_member_counts) == 16, "phj_member_counts layout");

int phj_join_member(phj_ctx* c, const phj_join_params* p, uint32_t sides, uint8_t* probe_mask, uint8_t* build_mask,
                    phj_join_result* r, phj_member_counts* n) {
    return join_member(c, p, sides, probe_mask, build_mask, r, n);
}

// ---- the retained key index (phj_lookup.h) ----
static_assert(sizeof(phj_index_info) == 40, "phj_index_info layout");

int phj_index_build(phj_ctx* c, const phj_join_params* p, phj_index** out, phj_join_result* r) {
    return index_build(c, p, 0, out, r);
}

int phj_index_build_ex(phj_ctx* c, const phj_join_params* p, uint32_t flags, phj_index** out, phj_join_result* r) {
    return index_build(c, p, flags, out, r);
}

int phj_index_flags_get(const phj_index* ix, uint32_t* flags) {
    if (!ix || !flags) return PHJ_ERR_INVALID;
    *flags = ix->flags;
    return PHJ_OK;
}

int phj_index_uniques(phj_ctx* c, const phj_index* ix, const int64_t** dev_first_rows, uint64_t* n) {
    if (!c || !ix || !dev_first_rows || !n) return PHJ_ERR_INVALID;
    *dev_first_rows = nullptr;
    *n = 0;
    if (c->group) return set_err(c, PHJ_ERR_STATE, "phj_index_uniques: single-device contexts only");
    if (ix->owner != c) return set_err(c, PHJ_ERR_INVALID, "phj_index_uniques: the index belongs to another context");
    if (!(ix->flags & PHJ_INDEX_ORDINALS)) return set_err(c, PHJ_ERR_STATE, "phj_index_uniques: index built without ordinals");
    *dev_first_rows = ix->distinct ? ix->first_rows : nullptr;
    *n = ix->distinct;
    return PHJ_OK;
}

int phj_index_encode(phj_ctx* c, const phj_index* ix, const int64_t* dev_keys, uint32_t key_stride, uint64_t n,
                     int64_t* out_codes, uint8_t* out_found, unsigned long long* dev_found_count) {
    return index_lookup(c, ix, dev_keys, key_stride, n, out_codes, out_found, dev_found_count, true);
}

int phj_index_accumulate(phj_ctx* c, const phj_index* ix, const int64_t* dev_keys, uint32_t key_stride,
                         const int64_t* dev_values, uint32_t value_stride, uint64_t n, unsigned long long* dev_counts,
                         int64_t* dev_sums, unsigned long long* dev_missing_count) {
    return index_accumulate(c, ix, dev_keys, key_stride, dev_values, value_stride, n, dev_counts, dev_sums, dev_missing_count);
}

int phj_index_info_get(const phj_index* ix, phj_index_info* out) {
    if (!ix || !out) return PHJ_ERR_INVALID;
    out->rows = ix->rows;
    out->distinct = ix->distinct;
    out->table_bytes = ix->bytes;
    out->nb = ix->g.nb;
    out->nbr = ix->g.nbr;
    out->rbits = ix->g.rbits;
    out->slots = kIxSlots;
    return PHJ_OK;
}

int phj_index_lookup(phj_ctx* c, const phj_index* ix, const int64_t* dev_keys, uint32_t key_stride, uint64_t n,
                     int64_t* out_rows, uint8_t* out_found, unsigned long long* dev_found_count) {
    return index_lookup(c, ix, dev_keys, key_stride, n, out_rows, out_found, dev_found_count);
}

void phj_index_destroy(phj_ctx* c, phj_index* ix) {
    if (!c || !ix) return;
    auto it = std::find(c->indexes.begin(), c->indexes.end(), ix);
    if (it == c->indexes.end()) return;
    c->indexes.erase(it);
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);   // lookups still in the stream read the table
    if (ix->tab) (void)hipFree(ix->tab);
    if (ix->first_rows) (void)hipFree(ix->first_rows);
    delete ix;
}

int phj_probe_pass1(phj_ctx* c, const phj_join_params* p, int64_t* keys, uint64_t n, uint32_t* bounds1,
                    uint32_t* nb1, int* codes) {
    if (!c) return PHJ_ERR_INVALID;
    if (c->group) return set_err(c, PHJ_ERR_STATE, "phj_probe_pass1 takes a single-device context");
    if (!p || !bounds1 || !nb1 || !codes || (n && !keys)) return set_err(c, PHJ_ERR_INVALID, "null argument");
    if (p->algo != PHJ_ALGO_RADIX) return set_err(c, PHJ_ERR_INVALID, "radix join parameters required");
    SideState& S = c->side[PHJ_SIDE_PROBE];
    if (n != S.n) return set_err(c, PHJ_ERR_INVALID, "n must be the probe relation's size");
    Plan asked, pl;   // pl: the LDS join's clusters, or the code tables' plan
    PHJ_TRY(make_plan(c, p, asked));
    if (radix_path(c, asked, S.n, c->side[PHJ_SIDE_BUILD].n, pl) == PHJ_PATH_PARTITIONED)
        return set_err(c, PHJ_ERR_STATE, "these params do not take the on-chip probe");
    PHJ_TRY(begin_call(c));
    if (!cols_native(c, S, pl, false)) PHJ_TRY(need_tuples(c, PHJ_SIDE_PROBE, false, "phj_probe_pass1"));   // (bound as columns)
    PHJ_TRY(partition_side(c, PHJ_SIDE_PROBE, pl, true));
    const uint32_t nt = S.nt2;
    PHJ_TRY(ensure(c, c->prep, (static_cast<size_t>(nt) + 1) * 4));
    PHJ_TRY(ensure(c, S.kB, std::max<uint64_t>(1, n) * 8));
    auto* off = static_cast<uint32_t*>(c->prep.p);
    hipLaunchKernelGGL(k_tile_counts<4096>, dim3(nt / 256 + 1), dim3(256), 0, c->ks, S.p2, nt, off);
    PHJ_LAUNCHED(c, "k_tile_counts");
    PHJ_TRY(scan_u32(c, off, nt + 1, 1, nt + 1));
    if (nt) {
        hipLaunchKernelGGL(k_gather_pass1<4096>, dim3(nt), dim3(256), 0, c->ks, S.p2, off, static_cast<int64_t*>(S.kB.p));
        PHJ_LAUNCHED(c, "k_gather_pass1");
    }
    uint32_t total = 0;
    PHJ_HIP(c, hipMemcpyAsync(&total, off + nt, 4, hipMemcpyDeviceToHost, c->ks));
    PHJ_HIP(c, hipMemcpyAsync(bounds1, S.bounds1.p, (static_cast<size_t>(pl.nb1) + 1) * 4, hipMemcpyDeviceToHost, c->ks));
    if (n) PHJ_HIP(c, hipMemcpyAsync(keys, S.kB.p, n * 8, hipMemcpyDeviceToHost, c->ks));
    PHJ_HIP(c, hipStreamSynchronize(c->ks));
    PHJ_TRY(check_chunk_errors(c));
    if (total != n) return set_err(c, PHJ_ERR_STATE, "pass-1 tiles hold " + std::to_string(total) + " keys, not " + std::to_string(n));
    *nb1 = pl.nb1;
    *codes = S.hcoded ? 1 : 0;
    return PHJ_OK;
}

int phj_debug_poison_chunk_table(phj_ctx* c, int side, const phj_join_params* p, int byte) {
    if (!c) return PHJ_ERR_INVALID;
    PHJ_TRY(check_side(c, side));
    if (c->group) return set_err(c, PHJ_ERR_STATE, "phj_debug_poison_chunk_table takes a single-device context");
    if (!p || p->algo != PHJ_ALGO_RADIX) return set_err(c, PHJ_ERR_INVALID, "radix join parameters required");
    PHJ_TRY(begin_call(c, 0, true));
    Plan asked, pl;
    PHJ_TRY(make_plan(c, p, asked));
    // the pass phj_join runs on this side: keys-only codes for the on-chip probes
    const bool p1_only = radix_path(c, asked, c->side[PHJ_SIDE_PROBE].n, c->side[PHJ_SIDE_BUILD].n, pl) != PHJ_PATH_PARTITIONED &&
                         side == PHJ_SIDE_PROBE;
    SideState& S = c->side[side];
    if (!S.ctab.p) {   // no pass has allocated it yet: size it for phj_join's pass
        struct DryScope {
            phj_ctx* c;
            ~DryScope() { c->dry = false; }
        } scope{c};
        c->dry = true;
        PHJ_TRY(partition_state(c, S, side == PHJ_SIDE_BUILD ? "R" : "S", pl, p1_only));
    }
    if (!S.ctab.p) return set_err(c, PHJ_ERR_STATE, "these params take no chunked pass on this side");
    PHJ_HIP(c, hipMemsetAsync(S.ctab.p, byte & 0xff, S.ctab.bytes, c->stream));
    PHJ_HIP(c, hipStreamSynchronize(c->stream));
    S.ctab_dirty = false;
    return PHJ_OK;
}

int phj_debug_poison_alloc(phj_ctx* c, int byte) {
    if (!c) return PHJ_ERR_INVALID;
    const int v = byte < 0 ? -1 : (byte & 0xff);
    c->poison = v;
    if (c->group)
        for (int i = 0; i < c->group->nlocal(); i++) c->group->mem[i]->poison = v;
    return PHJ_OK;
}

int phj_debug_preagg(phj_ctx* c, int mode, uint64_t* stats) {
    if (!c) return PHJ_ERR_INVALID;
    if (mode < -1 || mode > 2) return set_err(c, PHJ_ERR_INVALID, "mode is -1 (keep), 0 (auto), 1 (off) or 2 (forced)");
    if (stats) stats[0] = stats[1] = 0;
    if (c->group) return PHJ_OK;   // the member step does not pre-aggregate
    if (stats && c->hot_ran && c->hot.p) {
        (void)hipGetLastError();
        PHJ_HIP(c, hipSetDevice(c->device));
        PHJ_HIP(c, hipStreamSynchronize(c->stream));
        struct {
            uint32_t entries, mass;
            unsigned long long kept;
        } h{};
        const char* ctl = static_cast<const char*>(c->hot.p) + static_cast<size_t>(kHotCounters) * 4 +
                          static_cast<size_t>(c->side[PHJ_SIDE_PROBE].plan.nb1) * kHotPer * 16;
        PHJ_HIP(c, hipMemcpy(&h, ctl, sizeof(h), hipMemcpyDeviceToHost));
        if (h.entries != 0 && h.mass >= c->hot_min_mass) {   // the passes' own test
            stats[0] = h.entries;
            stats[1] = c->hot_n - h.kept;
        }
    }
    if (mode >= 0) c->hot_mode = mode;
    return PHJ_OK;
}

int phj_debug_fail_member(phj_ctx* c, int member) {
    if (!c) return PHJ_ERR_INVALID;
    if (!c->group) return set_err(c, PHJ_ERR_STATE, "phj_debug_fail_member takes a multi-device or rank context");
    if (member < -1 || member >= c->group->nlocal()) return set_err(c, PHJ_ERR_INVALID, "no such local member");
    c->group->fail_member = member;
    return PHJ_OK;
}

int phj_debug_exchange_block(phj_ctx* c, int member, int64_t* out, uint64_t elems) {
    if (!c || !out) return PHJ_ERR_INVALID;
    if (!c->group) return set_err(c, PHJ_ERR_STATE, "phj_debug_exchange_block takes a multi-device or rank context");
    Group& G = *c->group;
    if (member < 0 || member >= G.nlocal()) return set_err(c, PHJ_ERR_INVALID, "no such local member");
    const DevBuf& b = G.buf[member].recv;
    if (!b.p || b.bytes < static_cast<size_t>(G.world) * elems * 8) return set_err(c, PHJ_ERR_STATE, "no exchange block of that size");
    PHJ_HIP(c, hipSetDevice(G.mem[member]->device));
    PHJ_HIP(c, hipStreamSynchronize(G.mem[member]->aux));
    PHJ_HIP(c, hipMemcpy(out, own_block(G, member, elems), elems * 8, hipMemcpyDeviceToHost));
    return PHJ_OK;
}

int phj_hash_keys(phj_ctx* c, int hash, uint64_t seed, const int64_t* keys, uint64_t n, uint64_t* out) {
    if (!c) return PHJ_ERR_INVALID;
    if (c->group)
        return on_solo(c, "phj_hash_keys", [&](phj_ctx* m) { return phj_hash_keys(m, hash, seed, keys, n, out); });
    if (hash != PHJ_HASH_XXH3 && hash != PHJ_HASH_MURMUR3) return set_err(c, PHJ_ERR_INVALID, "unknown hash function");
    if (n == 0) return PHJ_OK;
    (void)hipGetLastError();
    PHJ_HIP(c, hipSetDevice(c->device));
    void *dk = nullptr, *dout = nullptr;
    PHJ_HIP(c, hipMalloc(&dk, n * 8));
    hipError_t e = hipMalloc(&dout, n * 8);
    if (e != hipSuccess) {
        (void)hipFree(dk);
        return set_err(c, PHJ_ERR_NOMEM, "hipMalloc failed");
    }
    int rc = PHJ_OK;
    do {
        if (hipMemcpy(dk, keys, n * 8, hipMemcpyHostToDevice) != hipSuccess) { rc = set_err(c, PHJ_ERR_HIP, "H2D"); break; }
        const uint32_t g = static_cast<uint32_t>((n + kBlock - 1) / kBlock);
        with_hash(hash, [&](auto h) {
            hipLaunchKernelGGL((k_hash_keys<decltype(h)::value>), dim3(g), dim3(kBlock), 0, c->ks, static_cast<int64_t*>(dk), n, seed, static_cast<uint64_t*>(dout));
        });
        if (hipGetLastError() != hipSuccess) { rc = set_err(c, PHJ_ERR_HIP, "k_hash_keys launch"); break; }
        if (hipStreamSynchronize(c->ks) != hipSuccess) { rc = set_err(c, PHJ_ERR_HIP, "sync"); break; }
        if (hipMemcpy(out, dout, n * 8, hipMemcpyDeviceToHost) != hipSuccess) { rc = set_err(c, PHJ_ERR_HIP, "D2H"); break; }
    } while (0);
    (void)hipFree(dk);
    (void)hipFree(dout);
    return rc;
}

}  // extern "C"
