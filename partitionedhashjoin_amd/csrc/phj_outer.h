// phj_outer.h — rows for tuples without a partner: the outer and anti joins
// of phj_join_rows for gfx950.
//
// A join kind is a set of row classes (phj.h PHJ_ROWS_*): the inner join's
// pair rows, one null row per probe tuple with no equal build key, one null
// row per build tuple with no equal probe key. All of it sits on the inner
// join's count / scan / emit scheme (phj_inner.h):
//   1. count: the inner join's count pass leaves pairs[i] per probe tuple, so
//      pairs[i] == 0 is "probe tuple without a partner"; with build-only rows
//      asked it also marks every build tuple it compared equal (BMARK, one
//      byte per build tuple, cleared before the launch);
//   2. k_rows_map turns pairs[i] into the probe tuple's row count, keeps the
//      partnerless tuples in a bitmap and counts them;
//   3. the inner join's offsets and emit pass run unchanged over those row
//      counts, then k_rows_fill stores the null row of each flagged tuple at
//      its (still untouched) first row;
//   4. the unhit build tuples are compacted behind the probe part: a count
//      per 4096-element block, scan_u32, a write kernel (k_mat_count /
//      k_mat_write's scheme over the build storage).
// With an empty side nothing is joined: k_rows_side copies the other side.
#pragma once

#include "phj_inner.h"

namespace phj {

// pairs[i] -> rows of probe tuple i: (PAIRS ? pairs[i] : 0) + (pairs[i] == 0),
// the second term being its null row. only[i / 64] bit (i % 64) = tuple i has
// no partner (every word up to ceil(n / 64) is written); *count += how many.
// One workgroup per compaction block, so the wave of element i is aligned to
// the bitmap word.
template <bool PAIRS>
__global__ __launch_bounds__(kBlock) void k_rows_map(uint32_t* pairs, uint64_t n, uint64_t* only,
                                                     unsigned long long* count) {
    __shared__ uint32_t red[kWaves];
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kMatBlock;
    uint32_t c = 0;
#pragma unroll
    for (uint32_t j = 0; j < kMatBlockItems; j++) {
        const uint64_t i = base + j * kBlock + threadIdx.x;
        const uint32_t p = i < n ? pairs[i] : 1u;
        const bool lone = p == 0;
        const uint64_t bal = __ballot(lone);
        if ((threadIdx.x & 63) == 0 && i < n) only[i >> 6] = bal;
        if (i < n) pairs[i] = (PAIRS ? p : 0u) + (lone ? 1u : 0u);
        c += lone ? 1u : 0u;
    }
    c = block_sum(c, red);
    if (threadIdx.x == 0 && c) atomicAdd(count, static_cast<unsigned long long>(c));
}

// The null row {id, null_payload, payload_b} of every probe tuple flagged in
// only[], at the tuple's first row first[i] (the scanned pairs[]). The probe
// side is AoS tuples (sk == nullptr: s_aos) or SoA columns (sk, sp).
// SINK = IndexSink (phj_join_indices): the row is {null_payload, the tuple's
// row number}: sp[i], the number the radix join's partitioning carried, or i
// itself when sp is null (NoPartitioning: storage order is input order). No
// key is read.
template <class SINK = JoinedRow*>
__global__ __launch_bounds__(kBlock) void k_rows_fill(const uint64_t* only, const uint32_t* first, uint64_t n,
                                                      const longlong2* s_aos, const int64_t* sk, const int64_t* sp,
                                                      int64_t null_payload, SINK out, uint32_t nrows) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kBlock;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride) {
        if (!((only[i >> 6] >> (i & 63)) & 1)) continue;
        const uint32_t row = first[i];
        if (row >= nrows) continue;
        if constexpr (kIndexSink<SINK>) {
            put_row(out, row, 0, null_payload, sp ? sp[i] : static_cast<int64_t>(i));
        } else {
            JoinedRow r;
            if (sk) {
                r.id = sk[i];
                r.payload_b = sp[i];
            } else {
                const longlong2 t = s_aos[i];
                r.id = t.x;
                r.payload_b = t.y;
            }
            r.payload_a = null_payload;
            out[row] = r;
        }
    }
}

// An empty other side: every tuple of rel is "only", its row out[i] in input
// order. build: rel is the build side ({id, payload, null}), else the probe
// side ({id, null, payload}).
// SINK = IndexSink (phj_join_indices): row i is {i, null} or {null, i}; rel is
// not read (it may be null: a side bound as columns).
template <class SINK = JoinedRow*>
__global__ __launch_bounds__(kBlock) void k_rows_side(const longlong2* rel, uint64_t n, int64_t null_payload,
                                                      bool build, SINK out) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kBlock;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride) {
        if constexpr (kIndexSink<SINK>) {
            const int64_t me = static_cast<int64_t>(i);
            put_row(out, static_cast<uint32_t>(i), 0, build ? me : null_payload, build ? null_payload : me);
        } else {
            const longlong2 t = rel[i];
            JoinedRow r;
            r.id = t.x;
            r.payload_a = build ? t.y : null_payload;
            r.payload_b = build ? null_payload : t.y;
            out[i] = r;
        }
    }
}

// Element i of the build storage holds a build tuple that no probe key
// marked. NP: the storage is the bucket table's slots, i = b * kNPSlots + s,
// of which s < min(fill, kNPSlots) hold a tuple; else the partitioned build
// relation's rows, all of them tuples.
template <bool NP>
__device__ __forceinline__ bool build_unhit(uint64_t i, uint64_t n, const uint8_t* hit, const NPBucket* tab) {
    if (i >= n) return false;
    if (NP) {
        const uint32_t b = static_cast<uint32_t>(i / kNPSlots), s = static_cast<uint32_t>(i % kNPSlots);
        if (s >= tab[b].fill) return false;   // (fill > kNPSlots once full: s < kNPSlots always)
    }
    return hit[i] == 0;
}

// Unhit build tuples per compaction block -> cnt[block] (cnt has nblocks + 1
// entries; the exclusive scan turns it into row offsets), *count += their sum.
template <bool NP>
__global__ __launch_bounds__(kBlock) void k_build_only_count(const uint8_t* hit, const NPBucket* tab, uint64_t n,
                                                             uint32_t* cnt, unsigned long long* count) {
    __shared__ uint32_t red[kWaves];
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kMatBlock;
    uint32_t c = 0;
#pragma unroll
    for (uint32_t j = 0; j < kMatBlockItems; j++)
        c += build_unhit<NP>(base + j * kBlock + threadIdx.x, n, hit, tab) ? 1u : 0u;
    c = block_sum(c, red);
    if (threadIdx.x == 0) {
        cnt[blockIdx.x] = c;
        if (c) atomicAdd(count, static_cast<unsigned long long>(c));
    }
}

// The rows {id, payload_a, null_payload} of one compaction block's unhit build
// tuples from out[row0 + offs[block]] on (k_mat_write's positions: wave
// ballots inside the block). NP: keys from the table's slots, payloads
// pays[i]; else keys[i], pays[i]. Rows from nrows on are not stored (the
// count kernel saw the same flags: there are none).
// SINK = IndexSink (phj_join_indices): {pays[i], null_payload}, pays[i] being
// the build tuple's row number; no key is read.
template <bool NP, class SINK = JoinedRow*>
__global__ __launch_bounds__(kBlock) void k_build_only_write(const uint8_t* hit, const NPBucket* tab, uint64_t n,
                                                             const int64_t* keys, const int64_t* pays,
                                                             int64_t null_payload, const uint32_t* offs,
                                                             SINK out, uint32_t row0, uint32_t nrows) {
    __shared__ uint32_t wcnt[kWaves];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kMatBlock;
    uint32_t row = row0 + offs[blockIdx.x];
    for (uint32_t j = 0; j < kMatBlockItems; j++) {
        const uint64_t i = base + j * kBlock + threadIdx.x;
        const bool lone = build_unhit<NP>(i, n, hit, tab);
        const uint64_t bal = __ballot(lone);
        const uint32_t before = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wcnt[wave] = __popcll(bal);
        __syncthreads();
        uint32_t wbase = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kWaves; w++) {
            const uint32_t v = wcnt[w];
            wbase += static_cast<uint32_t>(w) < wave ? v : 0u;
            total += v;
        }
        const uint32_t at = row + wbase + before;
        if (lone && at < nrows) {
            if constexpr (kIndexSink<SINK>) {
                put_row(out, at, 0, pays[i], null_payload);
            } else {
                JoinedRow r;
                r.id = NP ? tab[i / kNPSlots].key[i % kNPSlots] : keys[i];
                r.payload_a = pays[i];
                r.payload_b = null_payload;
                out[at] = r;
            }
        }
        row += total;
        __syncthreads();   // wcnt reused by the next round
    }
}

}  // namespace phj
