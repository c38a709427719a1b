// phj_lookup.h — the retained key index (phj_index_build / phj_index_lookup):
// key -> lowest build row that carries it, built once, looked up per batch.
//
// The table is np_home_r's geometry (phj_join.h): 2^rbits regions of nbr
// buckets, a code's region its low rbits, its home bucket inside the region
// from the high word, the walk bucket by bucket over the whole table, wrapping.
// What differs from the NoPartitioning bucket table is what a bucket holds:
//
//   IxBucket (64 B, one line): 5 hash codes, their 5 build rows (32 bits),
//   a fill count. A lookup that settles in its home bucket reads that line and
//   nothing else; np_tab + np_pays would be two random lines per hit.
//
//   - Codes, not keys: both hashes are bijections of the 64-bit keys
//     (phj_hash.h), so equal codes are equal keys, and the lookup compares the
//     code it computed anyway. Inside region r's LDS build every code ends in
//     r, so r ^ 1 marks an unclaimed LDS slot for the compare-and-swap; in the
//     table itself only `fill` says which slots are live, so no key value is
//     reserved: 0, -1, INT64_MIN and INT64_MAX are keys like any other.
//   - Each distinct code once, with the lowest row: find-or-claim at build
//     time. A key repeated a million times is one entry and lengthens no walk.
//
//   k_ix_build_region   : one workgroup per region of R partitioned by region
//                         with row numbers (partition_side, PaySrc::RowNumber):
//                         find-or-claim in LDS (64-bit compare-and-swap on the
//                         code, atomicMin on the row), whole buckets out; a
//                         tuple that walks past the region's end goes to the
//                         overflow list
//   k_ix_build_overflow : the overflow list, find-or-claim with device atomics
//                         from the next region's first bucket (rare; a hot key
//                         or crafted collisions make it long, never wrong)
//   k_ix_lookup         : k_np_member_probe's shape over these buckets: one
//                         coalesced int64 row per lane, optional found bytes
//                         and count
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "phj_hash.h"
#include "phj_join.h"
#include "phj_member.h"

namespace phj {

constexpr int kIxSlots = 5;                    // {code, row} entries of a bucket
constexpr uint32_t kIxNoRow = 0xffffffffu;     // row word of a slot nobody published (build rows stay below 2^30)
constexpr uint32_t kIxRegionBuckets = 1024;    // buckets per region at most: 64 KB of LDS, two workgroups per CU

struct alignas(64) IxBucket {
    uint64_t code[kIxSlots];
    uint32_t row[kIxSlots];
    uint32_t fill;   // live slots, 0 .. 5: slots [0, fill) hold a code and its lowest row
};
static_assert(sizeof(IxBucket) == 64, "one line per bucket");

// count[0]: distinct codes (slots claimed); count[1]: nonzero when the overflow
// pass gave up on a tuple (a table without room: never, by its sizing)
template <int HK>
__global__ __launch_bounds__(kBlock) void k_ix_build_region(const int64_t* keys, const int64_t* rows,
                                                            const uint32_t* bounds, NPHome g, IxBucket* tab,
                                                            uint64_t seed, uint32_t* ovf_n, ulonglong2* ovf,
                                                            uint32_t* ovf_b, unsigned long long* count) {
    extern __shared__ __attribute__((aligned(64))) unsigned char smem[];
    IxBucket* lb = reinterpret_cast<IxBucket*>(smem);
    const uint32_t nbr = g.nbr, r = blockIdx.x;
    const uint64_t E = static_cast<uint64_t>(r ^ 1u);   // no code of region r: it ends in r ^ 1 (rbits >= 1)
    for (uint32_t i = threadIdx.x; i < nbr * kIxSlots; i += kBlock) {
        lb[i / kIxSlots].code[i % kIxSlots] = E;
        lb[i / kIxSlots].row[i % kIxSlots] = kIxNoRow;
    }
    __syncthreads();
    const uint32_t lo = bounds[r], hi = bounds[r + 1];
    const size_t b0 = static_cast<size_t>(r) * nbr;
    constexpr int IT = 4;   // their loads and hashes before the LDS walks
    for (uint32_t i0 = lo + threadIdx.x; i0 < hi; i0 += IT * kBlock) {
        int64_t k[IT], v[IT];
#pragma unroll
        for (int j = 0; j < IT; j++) {
            const uint32_t i = i0 + j * kBlock;
            k[j] = i < hi ? keys[i] : 0;
            v[j] = i < hi ? rows[i] : 0;
        }
#pragma unroll
        for (int j = 0; j < IT; j++) {
            if (i0 + j * kBlock >= hi) break;
            const uint64_t c = hash64<HK>(static_cast<uint64_t>(k[j]), seed);
            const uint32_t row = static_cast<uint32_t>(v[j]);
            uint32_t b = static_cast<uint32_t>(((c >> 32) * static_cast<uint64_t>(nbr)) >> 32);
            bool placed = false;
            while (!placed) {
                // slots are claimed in order and never freed: the first slot that
                // is E, or already this code, decides
#pragma unroll
                for (int s = 0; s < kIxSlots && !placed; s++) {
                    unsigned long long* slot = reinterpret_cast<unsigned long long*>(&lb[b].code[s]);
                    unsigned long long cur = *reinterpret_cast<volatile unsigned long long*>(slot);
                    if (cur == E) cur = atomicCAS(slot, static_cast<unsigned long long>(E), static_cast<unsigned long long>(c));
                    if (cur == E || cur == c) {
                        if (*reinterpret_cast<volatile uint32_t*>(&lb[b].row[s]) > row) atomicMin(&lb[b].row[s], row);
                        placed = true;
                    }
                }
                if (!placed && ++b == nbr) {   // past the region: find-or-claim later, from the next region
                    const uint32_t o = atomicAdd(ovf_n, 1u);
                    ovf[o] = make_ulonglong2(c, row);
                    ovf_b[o] = static_cast<uint32_t>((b0 + nbr) % g.nb);
                    placed = true;
                }
            }
        }
    }
    __syncthreads();
    // whole buckets out: 4 lanes per 64-B bucket; the lane with the last quarter counts the live slots
    const uint4* src = reinterpret_cast<const uint4*>(smem);
    uint4* out = reinterpret_cast<uint4*>(tab + b0);
    uint32_t live = 0;
    for (uint32_t i = threadIdx.x; i < nbr * 4; i += kBlock) {
        uint4 q = src[i];
        if ((i & 3) == 3) {
            const IxBucket& B = lb[i >> 2];
            uint32_t f = 0;
#pragma unroll
            for (int s = 0; s < kIxSlots; s++) f += B.code[s] != E ? 1u : 0u;
            q.w = f;
            live += f;
        }
        out[i] = q;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) live += __shfl_down(live, o, 64);
    if ((threadIdx.x & 63) == 0 && live) atomicAdd(count, static_cast<unsigned long long>(live));
}

// The overflow list with device atomics, after k_ix_build_region in stream
// order. Every lane keeps one tuple and all 64 stay in one loop (no lane waits
// inside a branch another lane must leave first): per turn a lane reads its
// bucket; a slot that is claimed but not yet published (row still kIxNoRow)
// means "look again next turn"; its code among the published slots is a find
// (atomicMin on the row); a bucket with room is claimed by a compare-and-swap
// fill -> fill + 1, which only succeeds if nobody claimed since this lane
// looked, so the lane has seen every earlier slot; the winner stores the code
// and publishes with the row. One lane per wave tries a claim per turn: a
// crafted list has every lane at the same bucket, and 64 failing swaps per
// wave would queue at that one word. A full bucket sends the lane on.
__global__ __launch_bounds__(kBlock) void k_ix_build_overflow(const uint32_t* ovf_n, const ulonglong2* ovf,
                                                              const uint32_t* ovf_b, IxBucket* tab, uint32_t nb,
                                                              unsigned long long* count) {
    const uint32_t n = *ovf_n;
    if (n == 0) return;
    const unsigned long long max_turns = (static_cast<unsigned long long>(nb) + n) * 64 + 4096;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t rounded = (n + 63) & ~63u;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < rounded; i += gridDim.x * kBlock) {
        bool active = i < n;
        const ulonglong2 t = active ? ovf[i] : make_ulonglong2(0, 0);
        const uint64_t c = t.x;
        const uint32_t row = static_cast<uint32_t>(t.y);
        uint32_t b = active ? ovf_b[i] : 0;
        uint32_t walked = 0;
        unsigned long long turns = 0;
        while (__any(active)) {
            bool want = false;
            uint32_t f = 0;
            if (active) {
                IxBucket* B = tab + b;
                f = __hip_atomic_load(&B->fill, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
                const uint32_t m = f < kIxSlots ? f : kIxSlots;
                bool again = false, found = false;
                for (uint32_t s = 0; s < m && !again && !found; s++) {
                    const uint32_t rw = __hip_atomic_load(&B->row[s], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
                    if (rw == kIxNoRow) {
                        again = true;
                    } else if (__hip_atomic_load(&B->code[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == c) {
                        if (rw > row) atomicMin(&B->row[s], row);
                        found = true;
                    }
                }
                if (found) active = false;
                else if (!again) {
                    if (m < kIxSlots) want = true;
                    else if (++walked >= nb) {   // every bucket full without this code: no room (never, by the sizing)
                        atomicOr(count + 1, 1ull);
                        active = false;
                    } else b = b + 1 == nb ? 0 : b + 1;
                }
                if (active && ++turns > max_turns) {
                    atomicOr(count + 1, 1ull);
                    active = false;
                    want = false;
                }
            }
            const unsigned long long wants = __ballot(want);
            if (want && lane == static_cast<uint32_t>(__ffsll(static_cast<long long>(wants)) - 1)) {
                IxBucket* B = tab + b;
                if (atomicCAS(&B->fill, f, f + 1) == f) {
                    __hip_atomic_store(&B->code[f], c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(&B->row[f], row, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);   // publishes the slot
                    atomicAdd(count, 1ull);
                    active = false;
                }
            }
        }
    }
}

struct IxLookupArgs {
    const int64_t* keys;         // STRIDE 1: a key column; 2: the ids of a tuple array
    uint64_t n;
    const IxBucket* tab;
    NPHome g;
    uint64_t seed;
    int64_t* rows;               // out: the lowest build row of key i, or PHJ_NO_ROW
    uint8_t* found;              // out, optional: one byte per key
    unsigned long long* count;   // optional: found keys are added
    const int64_t* first;        // IxMode::RowsVia: first_rows of the ordinal index (phj_ordinal.h)
};

// What a slot's 32-bit word is and what the lookup writes: Rows, a plain index:
// the word is the row; Codes, an ordinal index (phj_ordinal.h): the word is the
// key's ordinal and is written as it is (phj_index_encode); RowsVia, an ordinal
// index asked for rows: one dependent read of first[ordinal] per hit.
enum class IxMode { Rows = 0, Codes = 1, RowsVia = 2 };

constexpr int kIxItems = kMemberItems;   // keys per lane and step (member_store's shape)

// k_np_member_probe's structure: nontemporal key loads, every home line
// requested before any compare, the walks batched (every pending key's next
// bucket in flight at once; a settled key re-reads its last bucket). A line is
// four 16-B loads: 64 registers of buckets per lane at four keys, so the kernel
// is built for 4 waves per SIMD (the compiler's resource report: 97-99 VGPRs,
// which allocate 104 and allow 4 waves either way; no scratch).
template <int HK, int STRIDE, IxMode MODE = IxMode::Rows>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_ix_lookup(IxLookupArgs a) {
    constexpr int ITEMS = kIxItems;
    const ulonglong2* tab2 = reinterpret_cast<const ulonglong2*>(a.tab);
    const uint32_t tid = threadIdx.x;
    const uint32_t nb = a.g.nb;
    const uint64_t n = a.n, seed = a.seed;
    uint32_t hits = 0;
    const uint64_t step = static_cast<uint64_t>(gridDim.x) * 256 * ITEMS;
    for (uint64_t base = static_cast<uint64_t>(blockIdx.x) * 256 * ITEMS; base < n; base += step) {
        uint64_t c[ITEMS];
        uint32_t vm = 0;
#pragma unroll
        for (int i = 0; i < ITEMS; i++) {   // the batch streams past the caches' allocate (it is read once)
            const uint64_t r = base + i * 256 + tid;
            const uint64_t ix = min(r, n - 1);
            c[i] = static_cast<uint64_t>(__builtin_nontemporal_load(a.keys + STRIDE * ix));
            vm |= (r < n ? 1u : 0u) << i;
        }
        uint32_t b[ITEMS], row[ITEMS];
        ulonglong2 v[ITEMS][4];
#pragma unroll
        for (int i = 0; i < ITEMS; i++) {
            c[i] = hash64<HK>(c[i], seed);
            b[i] = np_home_r(c[i], a.g);
#pragma unroll
            for (int w = 0; w < 4; w++) v[i][w] = tab2[4ull * b[i] + w];
        }
        // one bucket against one code: bit 0 = hit, bit 1 = the bucket is full (go on); *rw = the hit's row
        auto look = [](const ulonglong2(&q)[4], uint64_t code, uint32_t* rw) -> uint32_t {
            const uint32_t fill = static_cast<uint32_t>(q[3].y >> 32);
            const uint32_t h = (q[0].x == code ? 1u : 0u) | (q[0].y == code ? 2u : 0u) | (q[1].x == code ? 4u : 0u) |
                               (q[1].y == code ? 8u : 0u) | (q[2].x == code ? 16u : 0u);
            const uint32_t live = h & ((1u << (fill < kIxSlots ? fill : kIxSlots)) - 1u);
            const uint32_t rr = live & 1u    ? static_cast<uint32_t>(q[2].y)
                                : live & 2u  ? static_cast<uint32_t>(q[2].y >> 32)
                                : live & 4u  ? static_cast<uint32_t>(q[3].x)
                                : live & 8u  ? static_cast<uint32_t>(q[3].x >> 32)
                                             : static_cast<uint32_t>(q[3].y);
            if (live) *rw = rr;
            return (live ? 1u : 0u) | (fill >= kIxSlots ? 2u : 0u);
        };
        uint32_t hitm = 0, pend = 0;
#pragma unroll
        for (int i = 0; i < ITEMS; i++) {
            const uint32_t valid = (vm >> i) & 1u;
            row[i] = kIxNoRow;
            const uint32_t s = look(v[i], c[i], &row[i]);
            hitm |= (valid & s & 1u) << i;
            pend |= (valid & ((s & 1u) ^ 1u) & (s >> 1)) << i;
        }
        uint32_t walked = 0;   // a table of full buckets only ends the walk after one round
        while (pend && ++walked < nb) {
#pragma unroll
            for (int i = 0; i < ITEMS; i++) {
                if ((pend >> i) & 1u) b[i] = b[i] + 1 == nb ? 0 : b[i] + 1;
#pragma unroll
                for (int w = 0; w < 4; w++) v[i][w] = tab2[4ull * b[i] + w];
            }
#pragma unroll
            for (int i = 0; i < ITEMS; i++) {
                const uint32_t pi = (pend >> i) & 1u;
                uint32_t rw = kIxNoRow;
                const uint32_t s = look(v[i], c[i], &rw);
                if (pi & s & 1u) row[i] = rw;
                hitm |= (pi & s & 1u) << i;
                pend &= ~((pi & ((s & 1u) | ((s >> 1) ^ 1u))) << i);
            }
        }
        hits += __popc(hitm);
        if constexpr (MODE == IxMode::RowsVia) {   // every gather requested before any store
            int64_t fr[ITEMS];
#pragma unroll
            for (int i = 0; i < ITEMS; i++) fr[i] = (hitm >> i) & 1u ? a.first[row[i]] : int64_t{-1};
#pragma unroll
            for (int i = 0; i < ITEMS; i++)
                if ((vm >> i) & 1u) a.rows[base + i * 256 + tid] = fr[i];
        } else {
#pragma unroll
            for (int i = 0; i < ITEMS; i++)   // 8 B per lane: a wave instruction writes one 512-byte run
                if ((vm >> i) & 1u)
                    a.rows[base + i * 256 + tid] = (hitm >> i) & 1u ? static_cast<int64_t>(row[i]) : int64_t{-1};
        }
        if (a.found) member_store(a.found, base, tid, hitm, vm);
    }
    if (a.count) member_count(hits, a.count);
}

}  // namespace phj
