// phj_inner.h — the inner join with duplicate build keys for gfx950.
//
// phj_join / phj_join_materialize answer the reference's question: does the
// probe key have a build tuple (HashTable::Get stops at the first hit,
// LinearProbing.hpp:160-180). The inner join R ⋈ S has one row per (build
// tuple, probe tuple) pair with equal ids. Two passes over the same join, so
// nothing is allocated on the device and the set of rows is deterministic:
//   1. count: pairs[i] = number of build keys equal to probe tuple i's key
//      (i in the probe side's storage order), the total in a 64-bit counter;
//   2. offsets: per 4096-tuple block the sum of pairs[], an exclusive scan of
//      the block sums (scan_u32), then pairs[i] becomes the first row of
//      probe tuple i (block offset + exclusive prefix inside the block);
//   3. emit: the join again; every equal build key of probe tuple i stores
//      {id, payloadA, payloadB} at pairs[i], pairs[i] + 1, ...
// Rows are grouped by probe tuple, groups in the probe side's storage order.
// Rows are addressed with 32 bits: the host runs pass 2 and 3 only below
// 2^32 pairs (then no block sum can have wrapped either).
#pragma once

#include <type_traits>

#include "phj_mat.h"

// A/B builds only (make build/libphj_NAME.so HIPDEFS=-DPHJ_INNER_COOP=0): the
// radix join without the wave-cooperative compare of long buckets.
#ifndef PHJ_INNER_COOP
#define PHJ_INNER_COOP 1
#endif

namespace phj {

constexpr uint32_t kInnerWide = 64;   // k_inner_fused: bucket length from which the wave shares a probe key's compares
constexpr uint32_t kInnerWideLanes = 16;   // ... count pass: only while at most this many lanes have such a bucket
constexpr uint32_t kInnerHitBit = 0x80000000u;   // k_inner_fused, BMARK: lr[pos] = in-round index | this once compared equal

// Where an emitting kernel stores a row: the 24-B rows of phj_join_inner /
// phj_join_rows (JoinedRow*), or the two index columns of phj_join_indices
// (phj_index.h), whose joins carry row numbers as payloads: build_rows[at] and
// probe_rows[at], no id and no 24-B row. The sink is a template parameter
// whose default is the row pointer, so the instantiations of the row joins
// keep their arguments and their code.
struct IndexSink {
    int64_t* build_rows;
    int64_t* probe_rows;
};

__device__ __forceinline__ void put_row(JoinedRow* out, uint32_t at, int64_t id, int64_t pa, int64_t pb) {
    JoinedRow r;
    r.id = id;
    r.payload_a = pa;
    r.payload_b = pb;
    out[at] = r;
}

__device__ __forceinline__ void put_row(const IndexSink& out, uint32_t at, int64_t, int64_t pa, int64_t pb) {
    out.build_rows[at] = pa;
    out.probe_rows[at] = pb;
}

template <class SINK>
constexpr bool kIndexSink = std::is_same<SINK, IndexSink>::value;

// BMARK (the count pass of phj_join_rows with build-only rows, phj_outer.h):
// the join also says which build tuples met an equal probe key, one byte per
// build tuple, cleared by the host before the launch. A flag is only ever
// stored as 1 (several waves serve one partition, thousands of probe tuples
// one hot key), so no atomic and no order between the writers is needed.
// The count pass stores no rows: its `out` argument carries the flags, so the
// kernels' arguments, and with them the code of the instantiations
// phj_join_inner uses, stay as they were.

// The slots of one NoPartitioning bucket (its four 16-B words in q) equal to
// key; EMIT: their rows from out[row] on; BMARK: hit[b * kNPSlots + s] = 1 for
// each (tested first: a hot key's run is walked by thousands of probe tuples,
// whose steady state is then cached reads). Returns how many.
template <bool EMIT, bool BMARK, class SINK = JoinedRow*>
__device__ __forceinline__ uint32_t np_bucket_pairs(const longlong2 (&q)[4], uint32_t b, int64_t key,
                                                    const int64_t* pays, int64_t pb, SINK out, uint32_t row,
                                                    uint32_t nrows, uint8_t* hit) {
    int64_t ks[kNPSlots];
    const uint32_t fill = np_unpack(q, ks);
    const uint32_t c = fill < kNPSlots ? fill : kNPSlots;
    uint32_t n = 0;
#pragma unroll
    for (int s = 0; s < kNPSlots; s++) {
        if (static_cast<uint32_t>(s) < c && ks[s] == key) {
            if (EMIT && row + n < nrows) put_row(out, row + n, key, pays[static_cast<size_t>(b) * kNPSlots + s], pb);
            if (BMARK) {
                uint8_t* f = hit + static_cast<size_t>(b) * kNPSlots + s;
                if (*f == 0) *f = 1;
            }
            n++;
        }
    }
    return n;
}

// NoPartitioning inner join (k_np_probe_mark's structure). Every build tuple
// with S[i]'s key sits in the run of buckets from the key's home bucket to the
// first bucket that is not full (the build claims the first free slot walking
// that way, and nothing is ever removed), so the walk counts the equal slots
// of every bucket of that run, at most nb buckets.
// EMIT = false: pairs[i] = that number, *count += their sum.
// EMIT = true:  pairs[i] is probe tuple i's first row; rows beyond nrows are
//               not stored (the count pass saw the same table: there are none).
// BMARK (EMIT = false only): out holds the hit flags of the table's slots,
//               indexed like pays (b * kNPSlots + s).
// KEYS != 0 (phj_join_indices): S is read for its keys alone, in both passes,
// and probe tuple i's payload is i. KEYS = 1: S is a key column (int64 at
// stride 8, any 8-byte aligned base); KEYS = 2: 16-B tuples, their ids read at
// stride 16.
template <int HK, int KEYS, int IT>
__device__ __forceinline__ void np_probe_front_keys(const longlong2* S, uint64_t nS, uint64_t base, const NPBucket* tab,
                                                    NPHome g, uint64_t seed, longlong2 (&t)[IT], uint32_t (&b)[IT],
                                                    longlong2 (&q)[IT][4]) {
    static_assert(KEYS == 1 || KEYS == 2, "1: key column, 2: tuples");
    const int64_t* K = reinterpret_cast<const int64_t*>(S);
#pragma unroll
    for (int j = 0; j < IT; j++) {
        const uint64_t i = base + static_cast<uint64_t>(j) * kBlock + threadIdx.x;
        t[j].x = i < nS ? __builtin_nontemporal_load(K + i * KEYS) : 0;
        t[j].y = static_cast<int64_t>(i);
    }
#pragma unroll
    for (int j = 0; j < IT; j++) {
        b[j] = np_home_r(hash64<HK>(static_cast<uint64_t>(t[j].x), seed), g);
        const longlong2* bp = reinterpret_cast<const longlong2*>(tab + b[j]);
#pragma unroll
        for (int w = 0; w < 4; w++) q[j][w] = bp[w];
    }
}

template <int HK, bool EMIT, bool BMARK = false, class SINK = JoinedRow*, int KEYS = 0>
__global__ __launch_bounds__(kBlock) void k_np_inner(const longlong2* S, uint64_t nS, const NPBucket* tab,
                                                     const int64_t* pays, NPHome g, uint64_t seed, uint32_t* pairs,
                                                     unsigned long long* count, SINK out, uint32_t nrows) {
    static_assert(!(EMIT && BMARK), "hit flags are written by the count pass");
    static_assert(!BMARK || !kIndexSink<SINK>, "the hit flags travel in the row pointer");
    __shared__ unsigned long long red[kWaves];
    constexpr int IT = 4;   // as k_np_probe: every home bucket of a round requested before any compare
    uint8_t* hit = nullptr;
    if constexpr (BMARK) hit = reinterpret_cast<uint8_t*>(out);
    unsigned long long total = 0;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kBlock * IT;
    for (uint64_t base = static_cast<uint64_t>(blockIdx.x) * kBlock * IT; base < nS; base += stride) {
        longlong2 t[IT];
        uint32_t b[IT];
        longlong2 q[IT][4];
        if constexpr (KEYS != 0) np_probe_front_keys<HK, KEYS>(S, nS, base, tab, g, seed, t, b, q);
        else np_probe_front<HK, EMIT>(S, nS, base, tab, g, seed, t, b, q);
#pragma unroll
        for (int j = 0; j < IT; j++) {
            const uint64_t i = base + static_cast<uint64_t>(j) * kBlock + threadIdx.x;
            if (i >= nS) continue;
            const int64_t key = t[j].x;
            const uint32_t row = EMIT ? pairs[i] : 0u;
            uint32_t n = np_bucket_pairs<EMIT, BMARK>(q[j], b[j], key, pays, t[j].y, out, row, nrows, hit);
            bool full = static_cast<uint32_t>(q[j][3].y) >= kNPSlots;
            uint32_t bb = b[j];
            for (uint32_t step = 1; full && step < g.nb; step++) {   // full bucket: the run goes on
                bb = (bb + 1 == g.nb) ? 0 : bb + 1;
                const longlong2* bp = reinterpret_cast<const longlong2*>(tab + bb);
                longlong2 w[4];
#pragma unroll
                for (int x = 0; x < 4; x++) w[x] = bp[x];
                n += np_bucket_pairs<EMIT, BMARK>(w, bb, key, pays, t[j].y, out, row + n, nrows, hit);
                full = static_cast<uint32_t>(w[3].y) >= kNPSlots;
            }
            if (!EMIT) {
                pairs[i] = n;
                total += n;
            }
        }
    }
    if (!EMIT) {
        total = block_sum(total, red);
        if (total) atomicAdd(count, total);
    }
}

// Radix inner join: k_join_fused_mark's structure (one wave per (partition,
// S chunk) item, the partition's build keys in the wave's LDS CSR table in
// rounds of 256, each key's row in the partitioned build relation beside it).
// The table round, its scan and the block total are written out here as in
// k_join_fused_mark, not shared (phj_wave.h): with the round as a device
// function the count pass on a hot build key (thousands of rounds on one
// wave) measured 6 % slower, so this kernel's code stays as it was generated.
// A probe key is looked up in every round and compared with its whole bucket:
// no early exit. Its lane owns pairs[s] for the item, so the value is carried
// from round to round in memory (64 probe keys per lane: too many for
// registers). A bucket of kInnerWide keys or more (a hot build key: up to 256
// copies per round) is compared by all 64 lanes, 64 table keys at a time, with
// a ballot for the row positions: one lane would otherwise store the whole
// group row by row while 63 wait.
// EMIT = false: pairs[s] = equal build keys over all rounds (written for
//               every probe tuple of every item, also when the build
//               partition is empty), *a.count += their sum.
// EMIT = true:  pairs[s] is probe tuple s's first row on entry and the cursor
//               behind its rows written so far between rounds.
// BMARK (EMIT = false only): out holds the hit flags of the partitioned build
//               relation's rows. lr[] is free in the count pass, so it keeps
//               each table position's in-round index and, once a probe key
//               compared equal there (either compare path), kInnerHitBit;
//               after the round's probe loop each lane turns its RPL
//               positions' bits into the flags of build rows rlo + r0 + index.
// SINK = IndexSink (phj_join_indices, EMIT only): the payloads both sides
// carry are row numbers and go to the two index columns; the wide path's 64
// consecutive rows are then two contiguous 512-B stores.
template <int HK, bool EMIT, bool BMARK = false, class SINK = JoinedRow*>
__global__ __launch_bounds__(kBlock) void k_inner_fused(FusedArgs a, uint32_t* pairs, const int64_t* spays,
                                                        SINK out, uint32_t nrows) {
    constexpr int TCAP = 256, RPL = TCAP / 64, OCAP = TCAP / 2 + 1, KPL = 4;
    constexpr uint32_t SUB = 64 * KPL;
    static_assert(!(EMIT && BMARK), "hit flags are written by the count pass");
    static_assert(EMIT || !kIndexSink<SINK>, "the count pass stores no rows");
    __shared__ int64_t lk_all[kWaves][TCAP];
    __shared__ uint32_t lr_all[kWaves][TCAP];
    __shared__ uint32_t lo_all[kWaves][OCAP];
    __shared__ uint32_t cur_all[kWaves][OCAP];
    __shared__ unsigned long long red[kWaves];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int64_t* lk = lk_all[wave];
    uint32_t* lr = lr_all[wave];
    uint32_t* loffs = lo_all[wave];
    uint32_t* lcur = cur_all[wave];
    uint8_t* hitf = nullptr;
    if constexpr (BMARK) hitf = reinterpret_cast<uint8_t*>(out);
    const int64_t* rkeys = a.L.seg[0].keys;
    const int64_t* rpays = a.L.seg[0].pays;
    const uint32_t* rb = a.L.seg[0].bounds;
    unsigned long long total = 0;
    for (uint32_t item = blockIdx.x * kWaves + wave; item < a.nitems; item += gridDim.x * kWaves) {
        const FusedItem it = a.items[item];
        if (it.s_cnt == 0) continue;
        const uint32_t rlo = rb[it.p], m = rb[it.p + 1] - rlo;
        if (m == 0) {   // no build tuple: the item's probe tuples have no pairs
            if (!EMIT)
                for (uint32_t off = lane; off < it.s_cnt; off += 64) pairs[it.s_lo + off] = 0;
            continue;
        }
        const uint32_t nsub = (it.s_cnt + SUB - 1) / SUB;
        for (uint32_t r0 = 0; r0 < m; r0 += TCAP) {
            const uint32_t mr = min(static_cast<uint32_t>(TCAP), m - r0);
            const uint32_t nbk = table_buckets(mr);
            int64_t rk[RPL];
            uint32_t bk[RPL];
#pragma unroll
            for (int j = 0; j < RPL; j++) {
                const uint32_t f = j * 64 + lane;
                rk[j] = f < mr ? rkeys[rlo + r0 + f] : 0;
            }
            for (uint32_t i = lane; i < nbk; i += 64) lcur[i] = 0;
            wave_lds_sync();
#pragma unroll
            for (int j = 0; j < RPL; j++) {
                bk[j] = bucket_of(hash64<HK>(static_cast<uint64_t>(rk[j]), a.seed), nbk);
                if (static_cast<uint32_t>(j * 64) + lane < mr) atomicAdd(&lcur[bk[j]], 1u);
            }
            wave_lds_sync();
            uint32_t carry = 0;
            for (uint32_t base = 0; base < nbk; base += 64) {
                const uint32_t i = base + lane;
                const uint32_t v = i < nbk ? lcur[i] : 0u;
                uint32_t x = v;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const uint32_t y = __shfl_up(x, o, 64);
                    if (lane >= static_cast<uint32_t>(o)) x += y;
                }
                if (i < nbk) {
                    loffs[i] = carry + x - v;
                    lcur[i] = carry + x - v;
                }
                carry += __shfl(x, 63, 64);
            }
            if (lane == 0) loffs[nbk] = mr;
            wave_lds_sync();
#pragma unroll
            for (int j = 0; j < RPL; j++) {
                const uint32_t f = j * 64 + lane;
                if (f < mr) {
                    const uint32_t pos = atomicAdd(&lcur[bk[j]], 1u);
                    lk[pos] = rk[j];
                    if (EMIT) lr[pos] = rlo + r0 + f;
                    if (BMARK) lr[pos] = f;
                }
            }
            wave_lds_sync();
            const bool last = r0 + TCAP >= m;
            for (uint32_t sub = 0; sub < nsub; sub++) {
#pragma unroll
                for (int j = 0; j < KPL; j++) {
                    const uint32_t off = sub * SUB + j * 64 + lane;
                    const bool act = off < it.s_cnt;
                    const uint32_t s = it.s_lo + (act ? off : 0u);
                    const int64_t key = act ? a.skeys[s] : 0;
                    const uint32_t b = bucket_of(hash64<HK>(static_cast<uint64_t>(key), a.seed), nbk);
                    const uint32_t t0 = act ? loffs[b] : 0u, t1 = act ? loffs[b + 1] : 0u;
                    // a long bucket (a key with many copies in this round) is
                    // compared by the whole wave below, not by its own lane
                    // (every lane of the wave gets here: the item and round
                    // loops are per wave). Counting, many long buckets at once
                    // are cheaper lane by lane: they are the same LDS words.
                    uint64_t todo = __ballot(PHJ_INNER_COOP != 0 && t1 - t0 >= kInnerWide);
                    if (!EMIT && __popcll(todo) > static_cast<int>(kInnerWideLanes)) todo = 0;
                    const bool wide = (todo >> lane) & 1;
                    uint32_t n = 0, row = 0;
                    int64_t pb = 0;
                    if (EMIT && wide) {
                        row = pairs[s];
                        pb = spays[s];
                    }
                    if (!wide) {
                        for (uint32_t t = t0; t < t1; t++) {
                            if (lk[t] == key) {
                                if (EMIT) {
                                    if (n == 0) {
                                        row = pairs[s];
                                        pb = spays[s];
                                    }
                                    if (row + n < nrows) put_row(out, row + n, key, rpays[lr[t]], pb);
                                }
                                if (BMARK) {   // (lanes on one hot key store the same word)
                                    const uint32_t v = lr[t];
                                    if (!(v & kInnerHitBit)) lr[t] = v | kInnerHitBit;
                                }
                                n++;
                            }
                        }
                    }
                    while (todo) {
                        const int src = __ffsll(static_cast<unsigned long long>(todo)) - 1;
                        todo &= todo - 1;
                        const int64_t wkey = __shfl(key, src, 64);
                        const uint32_t w1 = __shfl(t1, src, 64);
                        const uint32_t wrow = __shfl(row, src, 64);
                        const int64_t wpb = __shfl(pb, src, 64);
                        uint32_t wn = 0;
                        for (uint32_t base = __shfl(t0, src, 64); base < w1; base += 64) {
                            const uint32_t t = base + lane;
                            const bool hit = t < w1 && lk[t] == wkey;
                            const uint64_t bal = __ballot(hit);
                            if (EMIT && hit) {   // 64 consecutive rows: one contiguous 1.5 KB store
                                const uint32_t at = wrow + wn + __popcll(bal & ((1ull << lane) - 1ull));
                                if (at < nrows) put_row(out, at, wkey, rpays[lr[t]], wpb);
                            }
                            if (BMARK && hit) {
                                const uint32_t v = lr[t];
                                if (!(v & kInnerHitBit)) lr[t] = v | kInnerHitBit;
                            }
                            wn += __popcll(bal);
                        }
                        if (lane == static_cast<uint32_t>(src)) n = wn;
                    }
                    if (act) {
                        if (EMIT) {
                            if (n && !last) pairs[s] = row + n;
                        } else {
                            if (r0 == 0) pairs[s] = n;
                            else if (n) pairs[s] += n;
                            total += n;
                        }
                    }
                }
            }
            if (BMARK) {
                wave_lds_sync();   // every lane's hit bits before they are read
#pragma unroll
                for (int j = 0; j < RPL; j++) {
                    const uint32_t pos = j * 64 + lane;
                    const uint32_t v = pos < mr ? lr[pos] : 0u;
                    if (v & kInnerHitBit) hitf[rlo + r0 + (v & ~kInnerHitBit)] = 1;
                }
            }
            wave_lds_sync();   // this round's LDS reads before the next round's stores
        }
    }
    if (!EMIT) {
        unsigned long long x = total;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
        if (lane == 0) red[wave] = x;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned long long t = 0;
            for (int w = 0; w < kWaves; w++) t += red[w];
            if (t) atomicAdd(a.count, t);
        }
    }
}

// Pairs per compaction block -> cnt[block] (cnt has nblocks + 1 entries; the
// exclusive scan turns it into the blocks' first rows). 32-bit sums: the host
// goes on only below 2^32 pairs in all.
__global__ __launch_bounds__(kBlock) void k_inner_blocksum(const uint32_t* pairs, uint64_t n, uint32_t* cnt) {
    block_sums<false>(pairs, n, cnt);
}

// pairs[i] -> first row of probe tuple i, in place: offs[block] plus the
// exclusive prefix of pairs[] inside the block. A thread takes 16 consecutive
// tuples; one wave scan of the thread sums and the wave totals give its base.
__global__ __launch_bounds__(kBlock) void k_inner_prefix(uint32_t* pairs, uint64_t n, const uint32_t* offs) {
    __shared__ uint32_t wsum[kWaves];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kMatBlock + threadIdx.x * kMatBlockItems;
    uint32_t v[kMatBlockItems];
    uint32_t sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < kMatBlockItems; j++) {
        v[j] = base + j < n ? pairs[base + j] : 0u;
        sum += v[j];
    }
    const uint32_t x = wave_scan_incl(sum, lane);
    if (lane == 63) wsum[wave] = x;
    __syncthreads();
    uint32_t row = offs[blockIdx.x] + x - sum;
#pragma unroll
    for (int w = 0; w < kWaves; w++) row += static_cast<uint32_t>(w) < wave ? wsum[w] : 0u;
#pragma unroll
    for (uint32_t j = 0; j < kMatBlockItems; j++) {
        if (base + j < n) pairs[base + j] = row;
        row += v[j];
    }
}

}  // namespace phj
