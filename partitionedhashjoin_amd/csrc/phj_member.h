// phj_member.h — membership joins (phj_join_member): which rows of a relation
// have a partner on the other side, as one byte per row in the caller's order.
//
// The schedule is the NoPartitioning count's (phj_table.h): R's hash codes are
// partitioned into 2^k region code tables (partition_build, k_np_ct_plan,
// k_ht_fill), S is read unpartitioned, in input order. That is the one path
// where the answer for row i comes out at lane i, so the mask is a coalesced
// write and nothing is scattered back.
//
//   k_np_member_probe : k_np_probe_ct's probe over keys alone (a key column, or
//                       ids at stride 16) that also writes each row's hit byte
//                       and, MARK, a one-byte mark for the slot it matched
//   k_member_build    : a pass over R in input order: every build key walks to
//                       its slot by the probe's rule and reads that slot's mark
//
// The matched slot is the same for every copy of a code and for both kernels:
// the first bucket on the walk from the home bucket that holds the code, .x
// before .y. k_ht_fill may store a repeated code in two slots; the rule makes
// the probes mark, and every build row of that key read, the one slot the
// walk meets first.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "phj_hash.h"
#include "phj_table.h"

namespace phj {

constexpr int kMemberItems = 4;   // rows per lane and step: 256 x 4 = 1024 rows per workgroup step

// The marking probe looks at a slot's mark before it stores it (1), or stores it
// for every hit (0; an A/B build, `make build/libphj_mstore.so
// HIPDEFS=-DPHJ_MEMBER_MARK_TEST=0`, scripts/member_bench.py). Under key skew
// most hits are of keys marked long ago: the look is a cache hit where the
// store of every hit queues on the hot keys' few lines.
#ifndef PHJ_MEMBER_MARK_TEST
#define PHJ_MEMBER_MARK_TEST 1
#endif

// Mask bytes of one workgroup step (256 lanes x 4 items): item i of lane tid is
// row base + i * 256 + tid; bit i of hitm is its answer, of vm whether the row
// exists. A byte store per lane: a wave instruction writes one 64-byte run,
// wherever the mask starts, and no byte outside [0, n). (Four rows per dword,
// one store instruction per wave and step, measured level with this: DESIGN.md
// §3 "Membership joins".)
__device__ __forceinline__ void member_store(uint8_t* mask, uint64_t base, uint32_t tid, uint32_t hitm, uint32_t vm) {
#pragma unroll
    for (int i = 0; i < kMemberItems; i++)
        if ((vm >> i) & 1u) mask[base + i * 256u + tid] = static_cast<uint8_t>((hitm >> i) & 1u);
}

__device__ __forceinline__ void member_mark(uint8_t* marks, uint32_t slot) {
    if (PHJ_MEMBER_MARK_TEST != 0 && marks[slot] != 0) return;
    marks[slot] = 1;
}

// A workgroup's 256 per-lane counts added to *count.
__device__ __forceinline__ void member_count(uint32_t x, unsigned long long* count) {
    __shared__ uint32_t red[4];
    const uint32_t tid = threadIdx.x;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
    if ((tid & 63) == 0) red[tid >> 6] = x;
    __syncthreads();
    if (tid == 0) {
        const unsigned long long t = static_cast<unsigned long long>(red[0]) + red[1] + red[2] + red[3];
        if (t) atomicAdd(count, t);
    }
}

struct MemberProbeArgs {
    const int64_t* keys;         // KEYS: S's key column; else S's tuples (ids at stride 16)
    uint64_t n;                  // rows of S
    const uint64_t* table;       // region code tables (k_ht_fill)
    const uint2* desc;
    const uint32_t* uni;         // {uniform?, cap} (k_np_ct_plan)
    uint32_t P;                  // regions (a power of two)
    uint32_t pad;
    uint64_t seed, e1;
    uint8_t* mask;               // null: count (and mark) only
    uint8_t* marks;              // MARK: one byte per table slot, cleared by the caller
    unsigned long long* count;
};

// k_np_probe_ct's structure (phj_table.h): nontemporal key loads, the loop
// instantiated per layout (descriptor-free uniform layout / desc[]), all home
// buckets in flight, batched walks. The marking form needs more than 64
// VGPRs: it is built for 7 waves per SIMD (72 registers) where the others keep
// k_np_probe_ct's 8, so that none of them touches scratch.
template <int HK, int ITEMS, bool KEYS, bool MARK>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(MARK ? 7 : 8))) void k_np_member_probe(MemberProbeArgs a) {
    static_assert(ITEMS == kMemberItems, "member_store takes kMemberItems rows per lane");
    const bool uniform = __builtin_amdgcn_readfirstlane(a.uni[0]) != 0;
    const uint32_t nbk = __builtin_amdgcn_readfirstlane(a.uni[1]) / 2;   // buckets per region (uniform)
    const ulonglong2* tab2 = reinterpret_cast<const ulonglong2*>(a.table);
    const uint32_t tid = threadIdx.x;
    const uint32_t P = a.P;
    const uint64_t nS = a.n, seed = a.seed, e1 = a.e1;
    uint32_t hits = 0;
    const uint64_t step = static_cast<uint64_t>(gridDim.x) * 256 * ITEMS;
    auto run = [&](auto UNI) {
        constexpr bool UNIFORM = decltype(UNI)::value;
        for (uint64_t base = static_cast<uint64_t>(blockIdx.x) * 256 * ITEMS; base < nS; base += step) {
            uint64_t c[ITEMS];
            uint32_t vm = 0;
#pragma unroll
            for (int i = 0; i < ITEMS; i++) {   // S streams past the caches' allocate (it is read once)
                const uint64_t r = base + i * 256 + tid;
                const uint64_t ix = min(r, nS - 1);
                c[i] = static_cast<uint64_t>(__builtin_nontemporal_load(a.keys + (KEYS ? ix : 2 * ix)));
                vm |= (r < nS ? 1u : 0u) << i;
            }
            uint32_t bb[ITEMS], bm[ITEMS], bk[ITEMS];
            ulonglong2 v[ITEMS];
            if constexpr (!UNIFORM) {   // every descriptor requested before any bucket
                uint2 ds[ITEMS];
#pragma unroll
                for (int i = 0; i < ITEMS; i++) {
                    c[i] = hash64<HK>(c[i], seed);
                    ds[i] = a.desc[static_cast<uint32_t>(c[i]) & (P - 1)];
                }
#pragma unroll
                for (int i = 0; i < ITEMS; i++) {
                    bb[i] = ds[i].x >> 1;
                    bm[i] = ds[i].y;
                }
            } else {
#pragma unroll
                for (int i = 0; i < ITEMS; i++) {
                    c[i] = hash64<HK>(c[i], seed);
                    bb[i] = (static_cast<uint32_t>(c[i]) & (P - 1)) * nbk;
                    bm[i] = nbk - 1;
                }
            }
#pragma unroll
            for (int i = 0; i < ITEMS; i++) {
                bk[i] = static_cast<uint32_t>(c[i] >> kHtBucketShift) & bm[i];
                v[i] = tab2[bb[i] + bk[i]];
            }
            uint32_t hitm = 0;   // bit i: item i exists and its key is in R
            uint32_t pend = 0;   // bit i: item i's bucket is full without a match
#pragma unroll
            for (int i = 0; i < ITEMS; i++) {
                const uint32_t valid = (vm >> i) & 1u;
                const uint64_t e = ht_empty(static_cast<uint32_t>(c[i]) & (P - 1), e1);
                const uint32_t hx = static_cast<uint32_t>(v[i].x == c[i]), hy = static_cast<uint32_t>(v[i].y == c[i]);
                const uint32_t hit = (hx | hy) & valid;
                hitm |= hit << i;
                if constexpr (MARK)
                    if (hit) member_mark(a.marks, 2u * (bb[i] + bk[i]) + (hx ^ 1u));   // (slots are 32-bit: build_ht)
                pend |= (valid & ((hx | hy) ^ 1u) & static_cast<uint32_t>(v[i].y != e)) << i;
            }
            // the walks: every pending item's next bucket in flight at once (loads
            // unconditional: a settled item re-reads its last bucket)
            while (pend) {
#pragma unroll
                for (int i = 0; i < ITEMS; i++) {
                    if ((pend >> i) & 1u) bk[i] = (bk[i] + 1) & bm[i];
                    v[i] = tab2[bb[i] + bk[i]];
                }
#pragma unroll
                for (int i = 0; i < ITEMS; i++) {
                    const uint32_t pi = (pend >> i) & 1u;
                    const uint64_t e = ht_empty(static_cast<uint32_t>(c[i]) & (P - 1), e1);
                    const uint32_t hx = static_cast<uint32_t>(v[i].x == c[i]), hy = static_cast<uint32_t>(v[i].y == c[i]);
                    const uint32_t hit = pi & (hx | hy);
                    const uint32_t done = pi & (hx | hy | static_cast<uint32_t>(v[i].y == e));
                    hitm |= hit << i;
                    if constexpr (MARK)
                        if (hit) member_mark(a.marks, 2u * (bb[i] + bk[i]) + (hx ^ 1u));   // (slots are 32-bit: build_ht)
                    pend &= ~(done << i);
                }
            }
            hits += __popc(hitm);
            if (a.mask) member_store(a.mask, base, tid, hitm, vm);
        }
    };
    if (uniform) run(std::true_type{});
    else run(std::false_type{});
    member_count(hits, a.count);
}

struct MemberBuildArgs {
    const int64_t* keys;         // KEYS: R's key column; else R's tuples (ids at stride 16)
    uint64_t n;                  // rows of R
    const uint64_t* table;
    const uint2* desc;
    const uint32_t* uni;
    uint32_t P;
    uint32_t pad;
    uint64_t seed, e1;
    uint8_t* mask;
    const uint8_t* marks;        // what the probes stored
    unsigned long long* count;   // count[0]: build rows with a partner; count[1]: nonzero when a build key was not found
};

// R in input order: each key walks from its home bucket to the first bucket
// holding its code (.x before .y: the slot the probes marked) and its mask byte
// is that slot's mark. A build key is always in its region's table; the walk is
// bounded by the region's bucket count all the same, and a key that is not
// found (a table that is not R's) raises count[1] instead of looping.
template <int HK, bool KEYS>
__global__ __launch_bounds__(256) void k_member_build(MemberBuildArgs a) {
    constexpr int ITEMS = kMemberItems;
    constexpr uint32_t kNone = 0xffffffffu;
    const bool uniform = __builtin_amdgcn_readfirstlane(a.uni[0]) != 0;
    const uint32_t nbk = __builtin_amdgcn_readfirstlane(a.uni[1]) / 2;
    const ulonglong2* tab2 = reinterpret_cast<const ulonglong2*>(a.table);
    const uint32_t tid = threadIdx.x;
    const uint32_t P = a.P;
    const uint64_t nR = a.n;
    uint32_t hits = 0, lost = 0;
    const uint64_t step = static_cast<uint64_t>(gridDim.x) * 256 * ITEMS;
    for (uint64_t base = static_cast<uint64_t>(blockIdx.x) * 256 * ITEMS; base < nR; base += step) {
        uint64_t c[ITEMS];
        uint32_t vm = 0;
#pragma unroll
        for (int i = 0; i < ITEMS; i++) {
            const uint64_t r = base + i * 256 + tid;
            const uint64_t ix = min(r, nR - 1);
            c[i] = static_cast<uint64_t>(a.keys[KEYS ? ix : 2 * ix]);
            vm |= (r < nR ? 1u : 0u) << i;
        }
        uint32_t bb[ITEMS], bm[ITEMS], bk[ITEMS], slot[ITEMS];
        ulonglong2 v[ITEMS];
#pragma unroll
        for (int i = 0; i < ITEMS; i++) {
            c[i] = hash64<HK>(c[i], a.seed);
            const uint32_t p = static_cast<uint32_t>(c[i]) & (P - 1);
            if (uniform) {
                bb[i] = p * nbk;
                bm[i] = nbk - 1;
            } else {
                const uint2 ds = a.desc[p];
                bb[i] = ds.x >> 1;
                bm[i] = ds.y;
            }
        }
#pragma unroll
        for (int i = 0; i < ITEMS; i++) {
            bk[i] = static_cast<uint32_t>(c[i] >> kHtBucketShift) & bm[i];
            v[i] = tab2[bb[i] + bk[i]];
        }
#pragma unroll
        for (int i = 0; i < ITEMS; i++) {
            const uint64_t e = ht_empty(static_cast<uint32_t>(c[i]) & (P - 1), a.e1);
            slot[i] = kNone;
            for (uint32_t it = 0; it <= bm[i]; it++) {   // at most every bucket of the region once
                if (it) v[i] = tab2[bb[i] + bk[i]];
                if (v[i].x == c[i]) slot[i] = 2 * (bb[i] + bk[i]);
                else if (v[i].y == c[i]) slot[i] = 2 * (bb[i] + bk[i]) + 1;
                if (slot[i] != kNone || v[i].y == e) break;
                bk[i] = (bk[i] + 1) & bm[i];
            }
        }
        uint32_t hitm = 0;
        uint8_t mk[ITEMS];
#pragma unroll
        for (int i = 0; i < ITEMS; i++) mk[i] = slot[i] != kNone ? a.marks[slot[i]] : uint8_t{0};
#pragma unroll
        for (int i = 0; i < ITEMS; i++) {
            const uint32_t valid = (vm >> i) & 1u;
            hitm |= (valid & (mk[i] != 0 ? 1u : 0u)) << i;
            lost |= valid & (slot[i] == kNone ? 1u : 0u);
        }
        hits += __popc(hitm);
        member_store(a.mask, base, tid, hitm, vm);
    }
    if (lost) atomicOr(a.count + 1, 1ull);
    member_count(hits, a.count);
}

}  // namespace phj
