// phj_hot.h — the hot table of the counting LDS join's probe side.
//
// A skewed probe side (Zipf s = 1.05: the 1024 hottest of 10M keys are 55 % of
// S) spends most of pass 1's writes and of the probe's reads on a few thousand
// keys, though the count only needs "how many S tuples carry the key" times
// "is it in R". So before S's pass 1 a strided sample of S is hashed and
// counted, and the codes sampled often enough enter a hot table; S's pass then
// counts a hot code into its entry's weight instead of writing it, and R's
// pass adds the weight of every hot code it meets to the join's count
// (k_chunk_codes_pipe HOT 1 / 2, phj_partition.h). A code that found no way
// takes the normal path, so any selection is exact.
//
// The table: per cluster digit of pass 1, kHotSub sets (the code's top bit)
// of kHotWays 64-bit codes, so a lookup needs only what the pass has computed
// and reads one 16-B set; a 64-bit weight per entry; two control words
// {entries, sampled keys covered}.
// Inputs without skew pay for none of this beyond a first look: in auto mode
// a first stage counts an eighth of the sample's tiles in LDS only (no global
// atomics: ~10 ns each per workgroup, the sample's whole cost) and adds up,
// per tile, the keys of counters that stand out inside that one tile; unless
// they cover a sixteenth of the stage's keys, the sample proper and the
// selection return at once (the table stays empty, the passes skip their lookups).
// An empty way holds a code of another cluster (0, or E of cluster 0: no key
// value is reserved). All of it, and the sample's counters, is written by
// k_hot_clear in every join: nothing is kept from the join before.
#pragma once

#include "phj_partition.h"

namespace phj {

constexpr uint32_t kHotTile = 4096;        // keys of one sample tile (one workgroup of k_hot_sample)
constexpr uint32_t kHotTiles = 128;        // sample tiles, spread evenly over S
constexpr uint32_t kHotCounters = 65536;   // sample counters (L2-resident, 256 KB), 16 bits each in the workgroups' LDS
constexpr uint32_t kHotThreshold = 16;     // sample count of a hot code at kHotTiles tiles (3.1e-5 of S)
constexpr uint32_t kHotHeavy = 8;          // codes sampled this many thresholds over are entered first
constexpr uint32_t kHotBlock = 1024;
constexpr uint32_t kHotStage = 8;          // auto mode: every 8th sample tile is the first stage
constexpr uint32_t kHotStageCount = 4;     // ... a tile's counter stands out at this count (4 of 4096 keys; uniform keys: none does)
constexpr uint32_t kHotCtlGo = 4, kHotCtlDone = 5, kHotCtlStage = 6, kHotCtlWords = 8;   // hot_ctl beyond kHotCtl*: 2-3 = the tuples S's pass wrote

struct HotArgs {
    const int64_t* rel;     // S: {id, payload} pairs
    uint32_t n, ntiles;     // tuples, kHotTile-tuple tiles
    uint32_t nsamp;         // sample tiles (<= ntiles)
    uint32_t thr;           // sample count of a hot code
    DigitFn f;              // pass 1's digit
    uint32_t nb;
    uint64_t e0;            // the empty way of set 0 (a code outside cluster 0); the other sets' is 0
    uint32_t* counters;     // [kHotCounters]
    unsigned long long* code;   // [nb][kHotPer]
    unsigned long long* w;      // [nb][kHotPer]
    uint32_t* ctl;          // kHotCtl*
    uint32_t staged;        // 1: two sample stages (k_hot_sample phase 1, 2), else one (phase 0) and the selection always runs
};

// device words of the state: counters, codes, weights, control words
__host__ __device__ constexpr size_t hot_state_bytes(uint32_t nb) {
    return static_cast<size_t>(kHotCounters) * 4 + static_cast<size_t>(nb) * kHotPer * 16 + kHotCtlWords * 4;
}

__device__ __forceinline__ uint32_t hot_counter_of(uint64_t code) {
    return static_cast<uint32_t>((code * 0x9E3779B97F4A7C15ull) >> 48);
}

// sample tile i of nsamp -> tile of S
__device__ __forceinline__ uint32_t hot_tile_of(const HotArgs& a, uint32_t i) {
    return static_cast<uint32_t>(static_cast<uint64_t>(i) * a.ntiles / a.nsamp);
}

__global__ __launch_bounds__(kHotBlock) void k_hot_clear(HotArgs a) {
    const uint32_t i0 = blockIdx.x * kHotBlock + threadIdx.x, step = gridDim.x * kHotBlock;
    for (uint32_t i = i0; i < kHotCounters; i += step) a.counters[i] = 0;
    for (uint32_t i = i0; i < a.nb * kHotPer; i += step) {
        a.code[i] = i < kHotPer ? a.e0 : 0ull;
        a.w[i] = 0;
    }
    if (i0 < kHotCtlWords) a.ctl[i0] = i0 == kHotCtlGo && !a.staged ? 1u : 0u;
}

// One workgroup per sample tile: its keys' codes counted in LDS (two 16-bit
// counters per word: a tile has 4096 keys, so no half carries), then the
// non-zero counters added to the global ones.
// phase 0: every sample tile; 1: the first look at tiles 0, 8, 16, .. (nothing
// global but the verdict); 2: every sample tile, if phase 1 said go
template <int HK>
__global__ __launch_bounds__(kHotBlock) void k_hot_sample(HotArgs a, uint32_t phase) {
    extern __shared__ __attribute__((aligned(16))) uint32_t hot_lds[];   // [kHotCounters / 2]
    const uint32_t tid = threadIdx.x;
    if (phase == 2 && __hip_atomic_load(&a.ctl[kHotCtlGo], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) return;   // workgroup-uniform
    const uint32_t b = blockIdx.x;
    const uint32_t si = phase == 1 ? b * kHotStage : b;
    if (si >= a.nsamp) return;
    for (uint32_t i = tid; i < kHotCounters / 2; i += kHotBlock) hot_lds[i] = 0;
    __syncthreads();
    const uint32_t lo = hot_tile_of(a, si) * kHotTile;
    const longlong2* rel = reinterpret_cast<const longlong2*>(a.rel);
#pragma unroll
    for (uint32_t i = 0; i < kHotTile / kHotBlock; i++) {
        const uint32_t ix = lo + i * kHotBlock + tid;
        if (ix >= a.n) continue;
        const uint32_t ci = hot_counter_of(hash64<HK>(static_cast<uint64_t>(rel[ix].x), a.f.seed));
        atomicAdd(&hot_lds[ci >> 1], 1u << ((ci & 1u) * 16));
    }
    __syncthreads();
    if (phase != 1) {
        for (uint32_t i = tid; i < kHotCounters / 2; i += kHotBlock) {
            const uint32_t v = hot_lds[i];
            if (v & 0xffffu) atomicAdd(&a.counters[2 * i], v & 0xffffu);
            if (v >> 16) atomicAdd(&a.counters[2 * i + 1], v >> 16);
        }
        return;
    }
    // the first look: this tile's keys in counters that stand out; the
    // stage's last workgroup turns the sum into the verdict
    __shared__ uint32_t sum;
    if (tid == 0) sum = 0;
    __syncthreads();
    uint32_t m = 0;
    for (uint32_t i = tid; i < kHotCounters / 2; i += kHotBlock) {
        const uint32_t v = hot_lds[i], c0 = v & 0xffffu, c1 = v >> 16;
        m += (c0 >= kHotStageCount ? c0 : 0u) + (c1 >= kHotStageCount ? c1 : 0u);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m += __shfl_xor(m, o, 64);
    if ((tid & 63) == 0 && m) atomicAdd(&sum, m);
    __syncthreads();
    if (tid == 0) {
        if (sum) atomicAdd(&a.ctl[kHotCtlStage], sum);
        __threadfence();
        if (atomicAdd(&a.ctl[kHotCtlDone], 1u) == gridDim.x - 1) {
            __threadfence();
            const uint32_t all = atomicAdd(&a.ctl[kHotCtlStage], 0u);
            const uint64_t cap = static_cast<uint64_t>(gridDim.x) * kHotTile, keys = a.n < cap ? a.n : cap;
            __hip_atomic_store(&a.ctl[kHotCtlGo], static_cast<uint64_t>(all) * 16 >= keys ? 1u : 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// The sample again: a code whose counter reached the threshold enters a set
// of its digit. The ways are tried in fixed order with a 64-bit
// compare-and-swap and never change once taken, so a code sits in one way at
// most; a set that is full drops the code. The heavy counters go first in
// every workgroup, so an overflowing set mostly keeps the larger counts. A
// hot code fills thousands of lanes (the hottest key of Zipf 1.05 is 7 % of
// them), and that many atomics on one set took 0.18 ms: per workgroup only
// the first lane of each counter (an LDS bitmap) goes to the table, so a set
// sees at most one lane per workgroup and code. Codes that only share a hot
// code's counter may enter too: harmless (a wasted way). The sampled keys the
// table covers are summed once per counter, by the lane that sets the
// counter's top bit.
constexpr uint32_t kHotClaimed = 0x80000000u;
template <int HK>
__global__ __launch_bounds__(kHotBlock) void k_hot_select(HotArgs a) {
    __shared__ uint32_t seen[kHotCounters / 32];   // counters a lane of this workgroup took
    const uint32_t tid = threadIdx.x;
    if (__hip_atomic_load(&a.ctl[kHotCtlGo], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) return;   // workgroup-uniform
    for (uint32_t i = tid; i < kHotCounters / 32; i += kHotBlock) seen[i] = 0;
    const uint32_t lo = hot_tile_of(a, blockIdx.x) * kHotTile;
    const longlong2* rel = reinterpret_cast<const longlong2*>(a.rel);
    constexpr uint32_t I = kHotTile / kHotBlock;
    uint64_t code[I];
    uint32_t cnt[I], ci[I];
#pragma unroll
    for (uint32_t i = 0; i < I; i++) {
        const uint32_t ix = lo + i * kHotBlock + tid;
        code[i] = 0;
        cnt[i] = 0;
        ci[i] = 0;
        if (ix >= a.n) continue;
        code[i] = hash64<HK>(static_cast<uint64_t>(rel[ix].x), a.f.seed);
        ci[i] = hot_counter_of(code[i]);
        cnt[i] = a.counters[ci[i]] & ~kHotClaimed;
    }
    __syncthreads();
    const uint32_t heavy = a.thr * kHotHeavy;
    uint32_t mass = 0;
    for (int round = 0; round < 2; round++) {
#pragma unroll
        for (uint32_t i = 0; i < I; i++) {
            const bool mine = round == 0 ? cnt[i] >= heavy : cnt[i] >= a.thr && cnt[i] < heavy;
            if (!mine) continue;
            const uint32_t bit = 1u << (ci[i] & 31u);
            if (atomicOr(&seen[ci[i] >> 5], bit) & bit) continue;   // another lane of the workgroup has this counter
            const uint32_t d = static_cast<uint32_t>(q_from_hash(code[i], a.f) >> a.f.shift) & a.f.dmask;
            if (d >= a.nb) continue;
            const unsigned long long empty = d == 0 ? a.e0 : 0ull;
            unsigned long long* set = a.code + static_cast<size_t>(d) * kHotPer + (code[i] >> 63) * kHotWays;
            for (uint32_t w = 0; w < kHotWays; w++) {
                unsigned long long v = __hip_atomic_load(&set[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (v == empty) v = atomicCAS(&set[w], empty, static_cast<unsigned long long>(code[i]));
                else if (v != code[i]) continue;
                if (v == empty) atomicAdd(&a.ctl[kHotCtlEntries], 1u);   // this lane entered it
                if (v == empty || v == code[i]) {
                    if (!(atomicOr(&a.counters[ci[i]], kHotClaimed) & kHotClaimed)) mass += cnt[i];
                    break;
                }
            }
        }
        __syncthreads();
    }
    if (mass) atomicAdd(&a.ctl[kHotCtlMass], mass);
}

}  // namespace phj
