// phj_ordinal.h — ordinals on the retained key index (phj_index_build_ex with
// PHJ_INDEX_ORDINALS; phj_index_uniques / _encode / _accumulate): a dense id
// per distinct key, 0 .. distinct-1 in the order of the keys' first rows
// (pandas.factorize of the build key column), and grouped counts and sums
// addressed by it.
//
// An ordinal index is the table of phj_lookup.h with each live slot's row word
// replaced by the key's ordinal, plus first_rows[ordinal] = that row: an encode
// that settles at home still reads one line, a row lookup pays one dependent
// read of first_rows.
//
// The build, after k_ix_build_overflow in stream order. No workgroup waits for
// another: the rank comes from a reduce / apply scan (scan_u32) between passes.
//
//   k_ix_ord_mark  : every live slot sets bit `row` of a bitmap of the build
//                    rows (cleared by the call): the distinct keys' first rows
//   k_ix_ord_popc  : rank[w] = popc(bitmap[w]); scan_u32 makes it exclusive
//   k_ix_ord_first : bit r set -> first_rows[rank[r >> 5] + popc(bits below r)]
//                    = r; adjacent lanes take adjacent bits, the stores ascend
//   k_ix_ord_apply : every live slot's row word becomes that same rank
//
//   k_ix_accumulate: the lookup's front; a found key adds 1 (and its value) to
//                    its ordinal's accumulators through a per-workgroup LDS
//                    cache, see below
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "phj_lookup.h"

namespace phj {

// Entries of a workgroup's accumulator cache in k_ix_accumulate (a power of
// two; 16 B of LDS each), or 0: every add is a global atomic (the A/B form,
// make build/libphj_accplain.so HIPDEFS=-DPHJ_IX_ACC_CACHE=0).
#ifndef PHJ_IX_ACC_CACHE
#define PHJ_IX_ACC_CACHE 2048
#endif
static_assert((PHJ_IX_ACC_CACHE & (PHJ_IX_ACC_CACHE - 1)) == 0 && PHJ_IX_ACC_CACHE <= 2048,
              "a power of two; more than 2048 entries leave no room for four workgroups per CU");

// The slots of 8 buckets per wave instruction: lane -> (bucket, slot), slots 5..7 idle.
__device__ __forceinline__ bool ix_live_slot(const IxBucket* tab, uint32_t nb, uint64_t t, uint32_t* b, uint32_t* s) {
    *b = static_cast<uint32_t>(t >> 3);
    *s = static_cast<uint32_t>(t & 7);
    return t >> 3 < nb && *s < kIxSlots && *s < tab[*b].fill;
}

__global__ __launch_bounds__(kBlock) void k_ix_ord_mark(const IxBucket* tab, uint32_t nb, uint32_t rows, uint32_t* bitmap) {
    uint32_t b, s;
    if (!ix_live_slot(tab, nb, static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x, &b, &s)) return;
    const uint32_t row = tab[b].row[s];
    if (row < rows) atomicOr(&bitmap[row >> 5], 1u << (row & 31));
}

__global__ __launch_bounds__(kBlock) void k_ix_ord_popc(const uint32_t* bitmap, uint32_t words, uint32_t* rank) {
    const uint32_t w = blockIdx.x * kBlock + threadIdx.x;
    if (w < words) rank[w] = __popc(bitmap[w]);
}

__device__ __forceinline__ uint32_t ix_rank_of(const uint32_t* bitmap, const uint32_t* rank, uint32_t row) {
    return rank[row >> 5] + __popc(bitmap[row >> 5] & ((1u << (row & 31)) - 1u));
}

__global__ __launch_bounds__(kBlock) void k_ix_ord_first(const uint32_t* bitmap, const uint32_t* rank, uint32_t rows,
                                                         int64_t* first_rows, uint64_t distinct) {
    const uint32_t row = blockIdx.x * kBlock + threadIdx.x;
    if (row >= rows || !((bitmap[row >> 5] >> (row & 31)) & 1u)) return;
    const uint32_t o = ix_rank_of(bitmap, rank, row);
    if (o < distinct) first_rows[o] = row;
}

__global__ __launch_bounds__(kBlock) void k_ix_ord_apply(IxBucket* tab, uint32_t nb, uint32_t rows, const uint32_t* bitmap,
                                                         const uint32_t* rank) {
    uint32_t b, s;
    if (!ix_live_slot(tab, nb, static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x, &b, &s)) return;
    const uint32_t row = tab[b].row[s];
    if (row < rows) tab[b].row[s] = ix_rank_of(bitmap, rank, row);
}

struct IxAccArgs {
    const int64_t* keys;          // STRIDE 1: a key column; 2: the ids of a tuple array
    uint64_t n;
    const IxBucket* tab;
    NPHome g;
    uint64_t seed;
    const int64_t* values;        // optional (with sums): the value of key i at i * vstride
    uint32_t vstride, pad;
    unsigned long long* counts;   // [distinct], the caller's: counts[ord] += 1
    unsigned long long* sums;     // [distinct], optional: sums[ord] += value, modulo 2^64
    unsigned long long* missing;  // optional: keys the index does not hold are added
};

constexpr uint32_t kIxAccEmpty = 0xffffffffu;   // tag of an unclaimed cache entry (ordinals stay below 2^30)
// keys per launch at most (the host splits longer batches): a cache entry's 32-bit count cannot wrap
constexpr uint64_t kIxAccLaunchKeys = 1ull << 31;

// k_ix_lookup's front (phj_lookup.h; repeated here, that kernel's text stays as
// it is): 256 lanes x 4 keys, nontemporal loads, every home line requested
// before any compare, batched walks. The slot's word is the key's ordinal.
//
// Adds. A Zipf batch sends several per cent of its keys to one ordinal, and
// one global word takes atomics one after another, so each workgroup sums what
// it can in LDS first: a direct-mapped cache of PHJ_IX_ACC_CACHE entries
// {tag, count, sum}, the entry chosen by the ordinal's low bits. A tag is
// claimed once, by compare-and-swap from empty, and never changes again: a key
// whose entry carries its ordinal adds with LDS atomics, a key whose entry is
// another ordinal's adds with global atomics at once. No eviction, so no
// protocol and no loop besides the bounded walk. The workgroup adds its live
// entries to the caller's accumulators once, at its end.
template <int HK, int STRIDE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_ix_accumulate(IxAccArgs a) {
    constexpr int ITEMS = kIxItems;
    constexpr uint32_t CACHE = PHJ_IX_ACC_CACHE;
    __shared__ uint32_t c_tag[CACHE ? CACHE : 1];
    __shared__ uint32_t c_cnt[CACHE ? CACHE : 1];
    __shared__ unsigned long long c_sum[CACHE ? CACHE : 1];
    const ulonglong2* tab2 = reinterpret_cast<const ulonglong2*>(a.tab);
    const uint32_t tid = threadIdx.x;
    const uint32_t nb = a.g.nb;
    const uint64_t n = a.n, seed = a.seed;
    const bool with_sums = a.sums != nullptr;
    if constexpr (CACHE != 0) {
        for (uint32_t i = tid; i < CACHE; i += 256) {
            c_tag[i] = kIxAccEmpty;
            c_cnt[i] = 0;
            c_sum[i] = 0;
        }
        __syncthreads();
    }
    uint32_t misses = 0;
    const uint64_t step = static_cast<uint64_t>(gridDim.x) * 256 * ITEMS;
    for (uint64_t base = static_cast<uint64_t>(blockIdx.x) * 256 * ITEMS; base < n; base += step) {
        uint64_t c[ITEMS];
        uint32_t vm = 0;
#pragma unroll
        for (int i = 0; i < ITEMS; i++) {
            const uint64_t r = base + i * 256 + tid;
            const uint64_t ix = min(r, n - 1);
            c[i] = static_cast<uint64_t>(__builtin_nontemporal_load(a.keys + STRIDE * ix));
            vm |= (r < n ? 1u : 0u) << i;
        }
        uint32_t b[ITEMS], ord[ITEMS];
        ulonglong2 v[ITEMS][4];
#pragma unroll
        for (int i = 0; i < ITEMS; i++) {
            c[i] = hash64<HK>(c[i], seed);
            b[i] = np_home_r(c[i], a.g);
#pragma unroll
            for (int w = 0; w < 4; w++) v[i][w] = tab2[4ull * b[i] + w];
        }
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
            ord[i] = kIxNoRow;
            const uint32_t s = look(v[i], c[i], &ord[i]);
            hitm |= (valid & s & 1u) << i;
            pend |= (valid & ((s & 1u) ^ 1u) & (s >> 1)) << i;
        }
        uint32_t walked = 0;
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
                if (pi & s & 1u) ord[i] = rw;
                hitm |= (pi & s & 1u) << i;
                pend &= ~((pi & ((s & 1u) | ((s >> 1) ^ 1u))) << i);
            }
        }
        misses += __popc(vm & ~hitm);
        unsigned long long val[ITEMS];
#pragma unroll
        for (int i = 0; i < ITEMS; i++) {   // the values stream past the caches too; a miss's value is not read
            val[i] = 0;
            if (with_sums && ((hitm >> i) & 1u))
                val[i] = static_cast<unsigned long long>(
                    __builtin_nontemporal_load(a.values + static_cast<uint64_t>(a.vstride) * (base + i * 256 + tid)));
        }
#pragma unroll
        for (int i = 0; i < ITEMS; i++) {
            if (!((hitm >> i) & 1u)) continue;
            const uint32_t o = ord[i];
            bool cached = false;
            if constexpr (CACHE != 0) {
                const uint32_t e = o & (CACHE - 1);
                uint32_t t = *reinterpret_cast<volatile uint32_t*>(&c_tag[e]);
                if (t == kIxAccEmpty) {
                    t = atomicCAS(&c_tag[e], kIxAccEmpty, o);
                    if (t == kIxAccEmpty) t = o;
                }
                if (t == o) {
                    atomicAdd(&c_cnt[e], 1u);
                    if (with_sums) atomicAdd(&c_sum[e], val[i]);
                    cached = true;
                }
            }
            if (!cached) {
                atomicAdd(&a.counts[o], 1ull);
                if (with_sums) atomicAdd(&a.sums[o], val[i]);
            }
        }
    }
    if constexpr (CACHE != 0) {
        __syncthreads();
        for (uint32_t e = tid; e < CACHE; e += 256) {
            const uint32_t t = c_tag[e];
            if (t == kIxAccEmpty) continue;
            atomicAdd(&a.counts[t], static_cast<unsigned long long>(c_cnt[e]));
            if (with_sums) atomicAdd(&a.sums[t], c_sum[e]);
        }
    }
    if (a.missing) member_count(misses, a.missing);
}

}  // namespace phj
