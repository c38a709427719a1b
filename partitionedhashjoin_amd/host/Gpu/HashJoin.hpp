// Drop-in GPU joiners with the reference's HashJoiner API:
//
//   RadixClustering::HashJoiner<HashTableFactory, HasherType>(Configuration, pool, hasher, factory)
//     .Run(tableA /*build*/, tableB /*probe*/, timer)       src/RadixCluster/HashJoin.hpp:92-135, 190-241
//   NoPartitioning::HashJoiner<HashTableFactory>(Configuration, pool, factory)
//     .Run(tableA, tableB, timer)                           src/NoPartitioning/HashJoin.hpp:15-41, 54-187
//
// The thread-pool slot of the reference constructors takes a Gpu::Device (one
// phj_ctx: device, stream, workspace). Run() hands &(*table)[0] / GetSize()
// to the C ABI (include/phj.h), runs partition / build / probe on the MI355X,
// drives the timer with the device-measured phase times and, like the
// reference, returns an empty Table<JoinedTuple> (counts only) unless
// GpuConfiguration::Materialize asks for the rows (phj_join_materialize:
// one JoinedTuple per matching probe tuple, copied back) or
// GpuConfiguration::MaterializeAll for the inner join's (phj_join_inner: one
// per pair of a build and a probe tuple with equal ids) or
// GpuConfiguration::RowClasses for an outer / anti join kind's (phj_join_rows:
// pair rows, and rows with NullPayload on the missing side for the probe and
// build tuples without a partner; the counts per class are added to the
// results as `pairs`, `probe_only`, `build_only`); the matched
// count (MaterializeAll: the pair count, RowClasses: the row count) is logged ("Joined N tuples", RadixCluster/HashJoin.hpp:320-321),
// added to the results as `matches`, and kept in GetNumberOfJoinedTuples().
// GpuConfiguration::Aggregate asks for the join's aggregates instead of rows
// (phj_join_aggregate: `pairs`, `probe_matched`, `sum_a`, `sum_b`, `sum_ab`
// added to the results; for groups also `groups` and `groups_checksum` over
// the group rows copied back); the returned table is empty, matches = pairs.
// GpuConfiguration::Member asks which rows have a partner on the other side
// (phj_join_member into masks held by a scratch context, copied back):
// `probe_matched`, `build_matched` and, per asked side, `probe_mask_checksum`
// / `build_mask_checksum` = Σ (i + 1) · mask[i] mod 2^64 are added to the
// results; the returned table is empty, matches = probe_matched.
// GpuConfiguration::Lookup asks for the retained key index instead of a join
// (internal::join_lookup: phj_index_build over tableA once, phj_index_lookup
// of tableB's keys in that many slices): `keys_looked_up`, `keys_found`,
// `index_distinct`, `index_build_us`, `lookup_batch_us` and
// `lookup_rows_checksum` = Σ (i + 1) · (row[i] + 1) mod 2^64 are added to the
// results; the returned table is empty, matches = keys_found.
// GpuConfiguration::Columns binds both relations as key / payload columns
// (phj_relation_to_columns) before whatever was asked for runs; the results'
// `layout` says which binding ran.
// GpuConfiguration::RowsAsIndices makes the rows of RowClasses / MaterializeAll
// another way (internal::join_by_indices): the key columns alone stay bound,
// phj_join_indices returns (build row, probe row) pairs and phj_gather_column
// composes the JoinedTuple columns from them; the results' `rows_as` says
// which way ran.
// C ABI errors surface as std::runtime_error / std::invalid_argument, which the
// CLI catches and turns into exit(1) (src/main.cpp:277-281).
#pragma once

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "Common/Configuration.hpp"
#include "Common/Hashers.hpp"
#include "Common/Logger.hpp"
#include "Common/Results.hpp"
#include "Common/Table.hpp"
#include "phj.h"

namespace Gpu {

// One phj_ctx: one HIP device, or several (the multi-GPU join: the relations
// are range-sharded across them, RCCL exchanges the partitioned build keys).
// The reference's thread pool (src/main.cpp:235-241) sits in this slot.
class Device {
   public:
    explicit Device(int device = 0) : m_device(device) {
        const int rc = phj_ctx_create_device(device, &m_ctx);
        if (rc != PHJ_OK) throw std::runtime_error("phj_ctx_create_device(" + std::to_string(device) + ") failed");
    }
    Device(const std::vector<int>& devices, uint32_t flags) {
        const int rc = phj_ctx_create_ex(static_cast<int>(devices.size()), devices.data(), flags, &m_ctx);
        if (rc != PHJ_OK)
            throw std::runtime_error("phj_ctx_create_ex(" + std::to_string(devices.size()) + " devices) failed");
        m_gpus = static_cast<int>(devices.size());
    }
    int NumberOfGpus() const { return m_gpus; }
    int DeviceId() const { return m_device; }   // of a single-device context
    ~Device() { phj_ctx_destroy(m_ctx); }
    Device(const Device&) = delete;
    Device& operator=(const Device&) = delete;

    phj_ctx* Get() const { return m_ctx; }

    void Check(int rc) const {
        if (rc == PHJ_OK) return;
        const std::string msg = phj_last_error(m_ctx);
        if (rc == PHJ_ERR_INVALID) throw std::invalid_argument(msg);
        throw std::runtime_error(msg);
    }

    void Upload(int side, const Common::Table<Common::Tuple>& t) {
        Check(phj_relation_upload(m_ctx, side, reinterpret_cast<const phj_tuple*>(t.Data()), t.GetSize()));
    }

   private:
    phj_ctx* m_ctx = nullptr;
    int m_gpus = 1;
    int m_device = 0;
};

namespace internal {

inline std::chrono::nanoseconds ms_to_ns(double ms) {
    return std::chrono::nanoseconds(static_cast<int64_t>(std::llround(ms * 1e6)));
}

// --rows indices: the rows of the join kind `classes` without a payload ever
// entering the join. Both relations are split into columns and only the key
// columns stay bound; phj_join_indices gives (build row, probe row) pairs;
// three gathers and a coalesce compose the rows' columns on the device:
//   payloadA = R.payload[build_rows], payloadB = S.payload[probe_rows] (null
//   where the side is missing), id = S.key[probe_rows], then R.key[build_rows]
//   into the same column with no null value (it keeps what the first wrote).
// The C ABI has no allocator: the three result columns are the columns of a
// scratch context's relations on the same device, read back as tuples.
inline std::shared_ptr<Common::Table<Common::JoinedTuple>> join_by_indices(Device& dev, const phj_join_params& p,
                                                                           phj_join_result& r, uint32_t classes,
                                                                           int64_t null_payload, phj_row_counts& n) {
    phj_ctx* c = dev.Get();
    const int64_t *rk = nullptr, *rp = nullptr, *sk = nullptr, *sp = nullptr;
    uint64_t nR = 0, nS = 0;
    dev.Check(phj_relation_to_columns(c, PHJ_SIDE_BUILD, 1));
    dev.Check(phj_relation_to_columns(c, PHJ_SIDE_PROBE, 1));
    dev.Check(phj_relation_columns(c, PHJ_SIDE_BUILD, &rk, &rp, &nR));
    dev.Check(phj_relation_columns(c, PHJ_SIDE_PROBE, &sk, &sp, &nS));
    if ((nR && !rp) || (nS && !sp)) throw std::runtime_error("--rows indices: a relation has no payload column to gather");
    // (the columns are context-owned and stay where they are: the join sees the keys alone)
    dev.Check(phj_relation_bind_columns(c, PHJ_SIDE_BUILD, rk, nullptr, nR));
    dev.Check(phj_relation_bind_columns(c, PHJ_SIDE_PROBE, sk, nullptr, nS));
    dev.Check(phj_join_indices(c, &p, classes, &r, &n));
    auto out = std::make_shared<Common::Table<Common::JoinedTuple>>(n.rows, Common::generate_uuid());
    if (n.rows == 0) return out;
    const int64_t *brows = nullptr, *prows = nullptr;
    uint64_t rows = 0;
    dev.Check(phj_joined_indices(c, &brows, &prows, &rows));
    if (rows != n.rows) throw std::runtime_error("phj_joined_indices: row count differs from the join's");
    Device scratch(dev.DeviceId());
    {
        const std::vector<int64_t> zeros(rows, 0);
        scratch.Check(phj_relation_upload_columns(scratch.Get(), PHJ_SIDE_BUILD, zeros.data(), zeros.data(), rows));
        scratch.Check(phj_relation_upload_columns(scratch.Get(), PHJ_SIDE_PROBE, zeros.data(), nullptr, rows));
    }
    const int64_t *id_c = nullptr, *pa_c = nullptr, *pb_c = nullptr;
    scratch.Check(phj_relation_columns(scratch.Get(), PHJ_SIDE_BUILD, &id_c, &pa_c, nullptr));
    scratch.Check(phj_relation_columns(scratch.Get(), PHJ_SIDE_PROBE, &pb_c, nullptr, nullptr));
    int64_t* id = const_cast<int64_t*>(id_c);
    int64_t* pa = const_cast<int64_t*>(pa_c);
    int64_t* pb = const_cast<int64_t*>(pb_c);
    const int64_t zero = 0;
    dev.Check(phj_gather_column(c, rp, nR, brows, rows, &null_payload, pa));
    dev.Check(phj_gather_column(c, sp, nS, prows, rows, &null_payload, pb));
    dev.Check(phj_gather_column(c, sk, nS, prows, rows, &zero, id));
    dev.Check(phj_gather_column(c, rk, nR, brows, rows, nullptr, id));
    std::vector<phj_tuple> t(rows);
    scratch.Check(phj_relation_download(scratch.Get(), PHJ_SIDE_BUILD, t.data(), rows));
    for (uint64_t i = 0; i < rows; i++) {
        (*out)[i].id = t[i].id;
        (*out)[i].payloadA = t[i].payload;
    }
    scratch.Check(phj_relation_download(scratch.Get(), PHJ_SIDE_PROBE, t.data(), rows));
    for (uint64_t i = 0; i < rows; i++) (*out)[i].payloadB = t[i].id;
    return out;
}

// --member: the masks of phj_join_member. The C ABI has no allocator: a mask
// is the key column of a scratch context's relation on the same device
// (ceil(n / 8) words), read back as tuples.
inline void join_member(Device& dev, const phj_join_params& p, phj_join_result& r, uint32_t sides,
                        Common::IHashJoinTimer& timer) {
    phj_ctx* c = dev.Get();
    Device scratch(dev.DeviceId());
    uint64_t n[2] = {0, 0};
    uint8_t* mask[2] = {nullptr, nullptr};
    const uint32_t bit[2] = {PHJ_MEMBER_BUILD, PHJ_MEMBER_PROBE};   // indexed by PHJ_SIDE_BUILD / PHJ_SIDE_PROBE
    for (int side : {PHJ_SIDE_BUILD, PHJ_SIDE_PROBE}) {
        (void)phj_relation_device_ptr(c, side, &n[side]);
        if (!(sides & bit[side]) || n[side] == 0) continue;
        const std::vector<int64_t> zeros((n[side] + 7) / 8, 0);
        scratch.Check(phj_relation_upload_columns(scratch.Get(), side, zeros.data(), nullptr, zeros.size()));
        const int64_t* col = nullptr;
        scratch.Check(phj_relation_columns(scratch.Get(), side, &col, nullptr, nullptr));
        mask[side] = reinterpret_cast<uint8_t*>(const_cast<int64_t*>(col));
    }
    phj_member_counts m{};
    dev.Check(phj_join_member(c, &p, sides, mask[PHJ_SIDE_PROBE], mask[PHJ_SIDE_BUILD], &r, &m));
    timer.AddResult("probe_matched", std::to_string(m.probe_matched));
    timer.AddResult("build_matched", std::to_string(m.build_matched));
    for (int side : {PHJ_SIDE_PROBE, PHJ_SIDE_BUILD}) {
        if (!(sides & bit[side])) continue;
        uint64_t sum = 0;
        if (mask[side]) {
            std::vector<phj_tuple> t((n[side] + 7) / 8);
            scratch.Check(phj_relation_download(scratch.Get(), side, t.data(), t.size()));
            for (uint64_t i = 0; i < n[side]; i++)
                sum += (i + 1) * ((static_cast<uint64_t>(t[i / 8].id) >> (8 * (i % 8))) & 0xffu);
        }
        timer.AddResult(side == PHJ_SIDE_PROBE ? "probe_mask_checksum" : "build_mask_checksum", std::to_string(sum));
    }
}

// --lookup BATCHES: a retained key index over tableA (phj_index_build, once),
// then tableB's keys looked up in BATCHES equal slices, enqueued back to back
// with one synchronise at the end (phj_index_lookup reads the bound probe
// relation's memory as a plain device pointer: the key column, or the tuples'
// ids at stride 2). The rows column and the found counter are columns of a
// scratch context (the C ABI has no allocator). r is the build's result with
// matches = the keys found (== the count join's matches) and probe_ms = the
// wall time of all lookups.
// --lookup-as codes | groups (as = 1 | 2): the index is built with ordinals
// (phj_index_build_ex). codes: phj_index_encode in place of the lookup, and
// `lookup_codes_checksum` = Σ (i + 1) · (code[i] + 1) mod 2^64. groups:
// phj_index_accumulate per slice with the probe payload as the value, into one
// pair of accumulators: `groups` (= the distinct keys), `groups_count_checksum`
// = Σ (j + 1) · count[j] and `groups_sum_checksum` = Σ (j + 1) · sum[j] mod
// 2^64; keys_found = the keys less the device's missing count.
inline void join_lookup_groups(Device& dev, const phj_join_params& p, phj_join_result& r, uint32_t batches,
                               Common::IHashJoinTimer& timer) {
    phj_ctx* c = dev.Get();
    uint64_t nS = 0;
    const int64_t *sk = nullptr, *sp = nullptr;
    uint32_t stride = 1;
    dev.Check(phj_relation_columns(c, PHJ_SIDE_PROBE, &sk, &sp, &nS));
    if (!sk) {
        sk = reinterpret_cast<const int64_t*>(phj_relation_device_ptr(c, PHJ_SIDE_PROBE, &nS));
        sp = sk ? sk + 1 : nullptr;
        stride = 2;
    }
    if (nS > 0 && !sp) throw std::runtime_error("--lookup-as groups sums the probe payloads: the probe side has none");
    phj_index* ix = nullptr;
    dev.Check(phj_index_build_ex(c, &p, PHJ_INDEX_ORDINALS, &ix, &r));
    phj_index_info info{};
    dev.Check(phj_index_info_get(ix, &info));
    const uint64_t d = info.distinct;
    Device scratch(dev.DeviceId());
    const std::vector<int64_t> zeros(d + 1, 0);   // {counts | missing}, {sums}
    scratch.Check(phj_relation_upload_columns(scratch.Get(), PHJ_SIDE_BUILD, zeros.data(), zeros.data(), zeros.size()));
    const int64_t *cnt_c = nullptr, *sum_c = nullptr;
    scratch.Check(phj_relation_columns(scratch.Get(), PHJ_SIDE_BUILD, &cnt_c, &sum_c, nullptr));
    auto* counts = reinterpret_cast<unsigned long long*>(const_cast<int64_t*>(cnt_c));
    int64_t* sums = const_cast<int64_t*>(sum_c);
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t b = 0; b < batches; b++) {
        const uint64_t lo = nS * b / batches, hi = nS * (b + 1) / batches;
        dev.Check(phj_index_accumulate(c, ix, sk ? sk + stride * lo : nullptr, stride, sp ? sp + stride * lo : nullptr, stride,
                                       hi - lo, counts, sums, counts + d));
    }
    dev.Check(phj_ctx_synchronize(c));
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    std::vector<phj_tuple> t(zeros.size());
    scratch.Check(phj_relation_download(scratch.Get(), PHJ_SIDE_BUILD, t.data(), t.size()));
    uint64_t csum = 0, ssum = 0, hits = 0;
    for (uint64_t j = 0; j < d; j++) {
        csum += (j + 1) * static_cast<uint64_t>(t[j].id);
        ssum += (j + 1) * static_cast<uint64_t>(t[j].payload);
        hits += static_cast<uint64_t>(t[j].id);
    }
    phj_index_destroy(c, ix);
    if (hits + static_cast<uint64_t>(t[d].id) != nS)
        throw std::runtime_error("--lookup-as groups: counts and the missing count do not add up to the keys");
    timer.AddResult("lookup_as", "groups");
    timer.AddResult("batches", std::to_string(batches));
    timer.AddResult("keys_looked_up", std::to_string(nS));
    timer.AddResult("keys_found", std::to_string(hits));
    timer.AddResult("index_rows", std::to_string(info.rows));
    timer.AddResult("index_distinct", std::to_string(info.distinct));
    timer.AddResult("index_table_bytes", std::to_string(info.table_bytes));
    timer.AddResult("index_build_us", std::to_string(static_cast<int64_t>(std::llround(r.build_ms * 1e3))));
    timer.AddResult("lookup_batch_us", std::to_string(static_cast<int64_t>(std::llround(ms * 1e3 / batches))));
    timer.AddResult("groups", std::to_string(d));
    timer.AddResult("groups_count_checksum", std::to_string(csum));
    timer.AddResult("groups_sum_checksum", std::to_string(ssum));
    r.matches = hits;
    r.probe_ms = ms;
}

inline void join_lookup(Device& dev, const phj_join_params& p, phj_join_result& r, uint32_t batches,
                        Common::IHashJoinTimer& timer, uint32_t as = 0) {
    if (as == 2) return join_lookup_groups(dev, p, r, batches, timer);
    phj_ctx* c = dev.Get();
    uint64_t nS = 0;
    const int64_t *sk = nullptr, *sp = nullptr;
    uint32_t stride = 1;
    dev.Check(phj_relation_columns(c, PHJ_SIDE_PROBE, &sk, &sp, &nS));
    if (!sk) {
        sk = reinterpret_cast<const int64_t*>(phj_relation_device_ptr(c, PHJ_SIDE_PROBE, &nS));
        stride = 2;
    }
    phj_index* ix = nullptr;
    if (as == 1) dev.Check(phj_index_build_ex(c, &p, PHJ_INDEX_ORDINALS, &ix, &r));
    else dev.Check(phj_index_build(c, &p, &ix, &r));
    phj_index_info info{};
    dev.Check(phj_index_info_get(ix, &info));
    Device scratch(dev.DeviceId());
    const std::vector<int64_t> zeros(std::max<uint64_t>(1, nS), 0);
    scratch.Check(phj_relation_upload_columns(scratch.Get(), PHJ_SIDE_BUILD, zeros.data(), nullptr, zeros.size()));
    scratch.Check(phj_relation_upload_columns(scratch.Get(), PHJ_SIDE_PROBE, zeros.data(), nullptr, 1));
    const int64_t *rows_c = nullptr, *cnt_c = nullptr;
    scratch.Check(phj_relation_columns(scratch.Get(), PHJ_SIDE_BUILD, &rows_c, nullptr, nullptr));
    scratch.Check(phj_relation_columns(scratch.Get(), PHJ_SIDE_PROBE, &cnt_c, nullptr, nullptr));
    int64_t* rows = const_cast<int64_t*>(rows_c);
    auto* cnt = reinterpret_cast<unsigned long long*>(const_cast<int64_t*>(cnt_c));
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t b = 0; b < batches; b++) {
        const uint64_t lo = nS * b / batches, hi = nS * (b + 1) / batches;
        if (as == 1) dev.Check(phj_index_encode(c, ix, sk ? sk + stride * lo : nullptr, stride, hi - lo, rows + lo, nullptr, cnt));
        else dev.Check(phj_index_lookup(c, ix, sk ? sk + stride * lo : nullptr, stride, hi - lo, rows + lo, nullptr, cnt));
    }
    dev.Check(phj_ctx_synchronize(c));
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    std::vector<phj_tuple> t(zeros.size());
    scratch.Check(phj_relation_download(scratch.Get(), PHJ_SIDE_BUILD, t.data(), t.size()));
    uint64_t sum = 0, hits = 0;
    for (uint64_t i = 0; i < nS; i++) {
        sum += (i + 1) * static_cast<uint64_t>(t[i].id + 1);
        hits += t[i].id != PHJ_NO_ROW ? 1 : 0;
    }
    phj_tuple found{};
    scratch.Check(phj_relation_download(scratch.Get(), PHJ_SIDE_PROBE, &found, 1));
    phj_index_destroy(c, ix);
    if (static_cast<uint64_t>(found.id) != hits)
        throw std::runtime_error("--lookup: the device's found count differs from the rows it wrote");
    if (as == 1) timer.AddResult("lookup_as", "codes");
    timer.AddResult("batches", std::to_string(batches));
    timer.AddResult("keys_looked_up", std::to_string(nS));
    timer.AddResult("keys_found", std::to_string(hits));
    timer.AddResult("index_rows", std::to_string(info.rows));
    timer.AddResult("index_distinct", std::to_string(info.distinct));
    timer.AddResult("index_table_bytes", std::to_string(info.table_bytes));
    timer.AddResult("index_build_us", std::to_string(static_cast<int64_t>(std::llround(r.build_ms * 1e3))));
    timer.AddResult("lookup_batch_us", std::to_string(static_cast<int64_t>(std::llround(ms * 1e3 / batches))));
    timer.AddResult(as == 1 ? "lookup_codes_checksum" : "lookup_rows_checksum", std::to_string(sum));
    r.matches = hits;
    r.probe_ms = ms;
}

// phj_join or, with rows requested, phj_join_materialize (one row per matching
// probe tuple) / phj_join_inner (all: one row per pair) + the rows copied into
// the returned table; with gpu.RowClasses, phj_join_rows of that kind
inline std::shared_ptr<Common::Table<Common::JoinedTuple>> join(Device& dev, const phj_join_params& p,
                                                                phj_join_result& r,
                                                                const Common::GpuConfiguration& gpu,
                                                                Common::IHashJoinTimer& timer) {
    const bool materialize = gpu.Materialize, all = gpu.MaterializeAll;
    if (gpu.Lookup != 0) {
        join_lookup(dev, p, r, gpu.Lookup, timer, gpu.LookupAs);
        return std::make_shared<Common::Table<Common::JoinedTuple>>(Common::generate_uuid());
    }
    if (gpu.Member != 0) {
        join_member(dev, p, r, gpu.Member, timer);
        return std::make_shared<Common::Table<Common::JoinedTuple>>(Common::generate_uuid());
    }
    if (gpu.Aggregate != 0) {
        phj_join_totals t{};
        dev.Check(phj_join_aggregate(dev.Get(), &p, gpu.Aggregate == 2 ? PHJ_AGG_GROUPS : 0u, &r, &t));
        timer.AddResult("pairs", std::to_string(t.pairs));
        timer.AddResult("probe_matched", std::to_string(t.probe_matched));
        timer.AddResult("sum_a", std::to_string(t.sum_a));
        timer.AddResult("sum_b", std::to_string(t.sum_b));
        timer.AddResult("sum_ab", std::to_string(t.sum_ab));
        if (gpu.Aggregate == 2) {
            uint64_t n = 0;
            (void)phj_group_rows(dev.Get(), &n);
            std::vector<phj_group_row> rows(n);
            dev.Check(phj_group_download(dev.Get(), rows.data(), n));
            uint64_t sum = 0;   // (order-free, as the rows' order is unspecified)
            for (const phj_group_row& g : rows)
                sum += static_cast<uint64_t>(g.id) * 3 + static_cast<uint64_t>(g.payload_a) * 5 + g.partners * 7 +
                       static_cast<uint64_t>(g.sum_b) * 11;
            timer.AddResult("groups", std::to_string(n));
            timer.AddResult("groups_checksum", std::to_string(sum));
        }
        return std::make_shared<Common::Table<Common::JoinedTuple>>(Common::generate_uuid());
    }
    if (gpu.RowsAsIndices && all) {
        phj_row_counts n{};
        return join_by_indices(dev, p, r, PHJ_ROWS_PAIRS, gpu.NullPayload, n);
    }
    if (gpu.RowClasses != 0) {
        phj_row_counts n{};
        std::shared_ptr<Common::Table<Common::JoinedTuple>> out;
        if (gpu.RowsAsIndices) {
            out = join_by_indices(dev, p, r, gpu.RowClasses, gpu.NullPayload, n);
        } else {
            dev.Check(phj_join_rows(dev.Get(), &p, gpu.RowClasses, gpu.NullPayload, &r, &n));
            out = std::make_shared<Common::Table<Common::JoinedTuple>>(n.rows, Common::generate_uuid());
            dev.Check(phj_joined_download(dev.Get(), reinterpret_cast<phj_joined*>(out->Data()), n.rows));
        }
        timer.AddResult("pairs", std::to_string(n.pairs));
        timer.AddResult("probe_only", std::to_string(n.probe_only));
        timer.AddResult("build_only", std::to_string(n.build_only));
        return out;
    }
    if (!materialize && !all) {
        dev.Check(phj_join(dev.Get(), &p, &r));
        return std::make_shared<Common::Table<Common::JoinedTuple>>(Common::generate_uuid());
    }
    static_assert(sizeof(Common::JoinedTuple) == sizeof(phj_joined), "JoinedTuple layout");
    dev.Check(all ? phj_join_inner(dev.Get(), &p, &r) : phj_join_materialize(dev.Get(), &p, &r));
    auto out = std::make_shared<Common::Table<Common::JoinedTuple>>(r.matches, Common::generate_uuid());
    dev.Check(phj_joined_download(dev.Get(), reinterpret_cast<phj_joined*>(out->Data()), r.matches));
    return out;
}

// --layout columns: both resident relations become key / payload columns on
// the device before the workspace is sized and the join runs
inline void apply_layout(Device& dev, const Common::GpuConfiguration& gpu) {
    if (!gpu.Columns) return;
    dev.Check(phj_relation_to_columns(dev.Get(), PHJ_SIDE_BUILD, 1));
    dev.Check(phj_relation_to_columns(dev.Get(), PHJ_SIDE_PROBE, 1));
}

inline void add_device_results(Common::IHashJoinTimer& timer, const phj_join_result& r, int gpus, bool columns = false,
                               bool indices = false) {
    timer.AddResult("matches", std::to_string(r.matches));
    timer.AddResult("gpus", std::to_string(gpus));
    timer.AddResult("exchange_us", std::to_string(static_cast<int64_t>(std::llround(r.exchange_ms * 1e3))));
    timer.AddResult("device_total_us", std::to_string(static_cast<int64_t>(std::llround(r.total_ms * 1e3))));
    timer.AddResult("algorithmic_bytes", std::to_string(r.algorithmic_bytes));
    timer.AddResult("layout", columns ? "columns" : "tuples");
    timer.AddResult("rows_as", indices ? "indices" : "payloads");
}

}  // namespace internal

namespace RadixClustering {

template <typename HashTableFactory, typename HasherType>
class HashJoiner {
   public:
    HashJoiner(::RadixClustering::Configuration configuration, std::shared_ptr<Device> device,
               const HasherType& hasher, const HashTableFactory& hashTableFactory,
               const Common::GpuConfiguration& gpu = Common::GpuConfiguration{})
        : m_configuration(configuration),
          m_device(std::move(device)),
          m_hasher(hasher),
          m_factory(hashTableFactory),
          m_gpu(gpu),
          m_logger(Common::GetNewLogger()) {
        Common::AddComponentAttributeToLogger(m_logger, "RadixPartitioning.HashJoiner");
    }

    // tableA is the build relation, tableB the probe relation (HashJoin.hpp:99)
    std::shared_ptr<Common::Table<Common::JoinedTuple>> Run(
        std::shared_ptr<Common::Table<Common::Tuple>> tableA, std::shared_ptr<Common::Table<Common::Tuple>> tableB,
        std::shared_ptr<Common::IHashJoinTimer> timer = std::make_shared<Common::NoOpHashJoinTimer>()) {
        m_device->Upload(PHJ_SIDE_BUILD, *tableA);
        m_device->Upload(PHJ_SIDE_PROBE, *tableB);
        return RunResident(timer);
    }

    // Join the relations already resident on the device (uploaded or generated there).
    std::shared_ptr<Common::Table<Common::JoinedTuple>> RunResident(
        std::shared_ptr<Common::IHashJoinTimer> timer = std::make_shared<Common::NoOpHashJoinTimer>()) {
        phj_join_params p{};
        p.algo = PHJ_ALGO_RADIX;
        p.hash = HasherType::kKind;
        p.hash_seed = m_hasher.Seed();
        p.flags = HashTableFactory::kTableFlags;   // the factory's table kind
        if (m_gpu.RadixBits[0] > 0) {
            p.num_partitions = 0;
            p.radix_bits[0] = static_cast<uint8_t>(m_gpu.RadixBits[0]);
            p.radix_bits[1] = static_cast<uint8_t>(m_gpu.RadixBits[1]);
        } else {
            if (m_configuration.NumberOfPartitions == 0 || m_configuration.NumberOfPartitions > 0xffffffffull)
                throw std::invalid_argument("number of partitions must be in [1, 2^32)");
            p.num_partitions = static_cast<uint32_t>(m_configuration.NumberOfPartitions);
        }
        LOG(m_logger, Common::debug) << "Starting hash partitioning.";
        phj_join_result r;
        std::memset(&r, 0, sizeof(r));
        // workspace allocation stays outside the timed phases, as the reference's
        // partitioned-table allocation does (RadixCluster/HashJoin.hpp:195-198)
        internal::apply_layout(*m_device, m_gpu);
        m_device->Check(phj_prepare(m_device->Get(), &p));
        auto joined = internal::join(*m_device, p, r, m_gpu, *timer);
        // partition: wall of both partition pipelines; build / probe: device phases
        timer->SetPartitionPhaseDuration(internal::ms_to_ns(r.partition_ms));
        timer->SetBuildPhaseDuration(internal::ms_to_ns(r.build_ms));
        timer->SetProbePhaseDuration(internal::ms_to_ns(r.probe_ms));
        internal::add_device_results(*timer, r, m_device->NumberOfGpus(), m_gpu.Columns, m_gpu.RowsAsIndices);
        timer->AddResult("partitions", std::to_string(r.num_partitions));
        m_joined = r.matches;
        m_last = r;
        LOG(m_logger, Common::debug) << "Joined  " << r.matches << " tuples";
        LOG(m_logger, Common::debug) << "Finished hash partitioning.";
        return joined;
    }

    uint64_t GetNumberOfJoinedTuples() const { return m_joined; }
    const phj_join_result& GetLastResult() const { return m_last; }

   private:
    ::RadixClustering::Configuration m_configuration;
    std::shared_ptr<Device> m_device;
    HasherType m_hasher;
    HashTableFactory m_factory;
    Common::GpuConfiguration m_gpu;
    Common::LoggerType m_logger;
    uint64_t m_joined = 0;
    phj_join_result m_last{};
};

}  // namespace RadixClustering

namespace NoPartitioning {

template <typename HashTableFactory>
class HashJoiner {
   public:
    HashJoiner(::NoPartitioning::Configuration configuration, std::shared_ptr<Device> device,
               const HashTableFactory& hashTableFactory, const Common::GpuConfiguration& gpu = Common::GpuConfiguration{})
        : m_configuration(configuration),
          m_device(std::move(device)),
          m_factory(hashTableFactory),
          m_gpu(gpu),
          m_logger(Common::GetNewLogger()) {
        Common::AddComponentAttributeToLogger(m_logger, "NoPartitioning.HashJoiner");
    }

    std::shared_ptr<Common::Table<Common::JoinedTuple>> Run(
        std::shared_ptr<Common::Table<Common::Tuple>> tableA, std::shared_ptr<Common::Table<Common::Tuple>> tableB,
        std::shared_ptr<Common::IHashJoinTimer> timer = std::make_shared<Common::NoOpHashJoinTimer>()) {
        m_device->Upload(PHJ_SIDE_BUILD, *tableA);
        m_device->Upload(PHJ_SIDE_PROBE, *tableB);
        return RunResident(timer);
    }

    std::shared_ptr<Common::Table<Common::JoinedTuple>> RunResident(
        std::shared_ptr<Common::IHashJoinTimer> timer = std::make_shared<Common::NoOpHashJoinTimer>()) {
        using Hasher = typename HashTableFactory::Hasher;
        phj_join_params p{};
        p.algo = PHJ_ALGO_NO_PARTITIONING;
        p.hash = Hasher::kKind;
        p.hash_seed = m_factory.GetHasher().Seed();
        p.table_ratio = m_gpu.TableRatio;
        LOG(m_logger, Common::debug) << "Starting hash partitioning.";
        phj_join_result r;
        std::memset(&r, 0, sizeof(r));
        // workspace allocation stays outside the timed phases, as the reference's
        // partitioned-table allocation does (RadixCluster/HashJoin.hpp:195-198)
        internal::apply_layout(*m_device, m_gpu);
        m_device->Check(phj_prepare(m_device->Get(), &p));
        auto joined = internal::join(*m_device, p, r, m_gpu, *timer);
        timer->SetBuildPhaseDuration(internal::ms_to_ns(r.build_ms));
        // the reference's probe figure runs from the build start (Results.hpp:202)
        timer->SetProbePhaseDuration(internal::ms_to_ns(r.build_ms + r.probe_ms));
        timer->SetPartitionPhaseDuration(std::chrono::nanoseconds(0));
        internal::add_device_results(*timer, r, m_device->NumberOfGpus(), m_gpu.Columns, m_gpu.RowsAsIndices);
        timer->AddResult("probe_only_us", std::to_string(static_cast<int64_t>(std::llround(r.probe_ms * 1e3))));
        m_joined = r.matches;
        m_last = r;
        LOG(m_logger, Common::debug) << "Joined " << r.matches << " tuples.";
        LOG(m_logger, Common::debug) << "Finished hash partitioning.";
        return joined;
    }

    uint64_t GetNumberOfJoinedTuples() const { return m_joined; }
    const phj_join_result& GetLastResult() const { return m_last; }

   private:
    ::NoPartitioning::Configuration m_configuration;
    std::shared_ptr<Device> m_device;
    HashTableFactory m_factory;
    Common::GpuConfiguration m_gpu;
    Common::LoggerType m_logger;
    uint64_t m_joined = 0;
    phj_join_result m_last{};
};

}  // namespace NoPartitioning
}  // namespace Gpu
