// phj_hot.h — the hot table of the counting LDS join's probe side.
//
// A skewed probe side (Zipf s = 1.05: the 1024 hottest of 10M keys are 55 % of
// S) spends most of pass 1's writes and of the probe's reads on a few thousand
// keys, though the count only needs "how many S tuples carry the key" times
// "is it in R". So before S's pass 1 a strided sample of S is hashed and
// counted, and the codes sampled often enough enter a hot table; S's pass then
// counts a hot code into its entry's weight instead of writing it
// (k_chunk_codes_pipe HOT 1, phj_partition.h). A hot entry is then a probe
// code that carries a weight, and the LDS join resolves it where it answers
// the same question for every other S code (phj_cluster.h): the workgroup of
// k_cluster_probe that owns a cluster (its range holds the cluster's first S
// tile) looks the cluster's entries up in the table it has just built and
// adds the weights of those found to its hits; k_cluster_probe_big does it
// for the clusters that kernel never builds (an HBM table, or no S tile left:
// then R's codes are scanned). R's codes are read no second time. R's pass 1
// has no part in it, so R's chain needs nothing of S's. A code that found no
// way takes the normal path, so any selection is exact.
//
// The table: per cluster digit of pass 1, kHotSub sets (the code's top bit)
// of kHotWays 64-bit codes, so a lookup needs only what the pass has computed
// and reads one 16-B set; a 64-bit weight per entry; two control words
// {entries, sampled keys covered}.
// The prologue is narrow (at most kHotTiles / kHotTilesPerWg = 32 workgroups
// at a time) so that it can share the chip with R's pass 1: the sample counts
// kHotTilesPerWg tiles per workgroup in LDS and flushes once; every sampled
// lane also leaves its code in its counter's word of a representative array
// (plain stores, the last writer wins), and one workgroup (k_hot_select)
// reads the counters, takes the representative of every counter at or above
// the threshold and builds the table in LDS. The representative may be a cold
// code that shares a hot code's counter: the hot code is then not entered.
// Inputs without skew pay for none of this beyond the LDS count: in auto mode
// a workgroup of the sample looks at its own LDS counters before anything
// global (the global atomics, ~10 ns each per workgroup, are the sample's
// whole cost) and adds up the keys of counters that stand out among the keys
// it counted; unless they cover a sixteenth of them, it leaves no global trace
// at all. A workgroup that goes on stores its representatives, flushes its
// counters and adds its vote to a control word; without a vote the selection
// writes an empty table at once (the pass skips its lookups), else it works
// on what was flushed (the coverage test of S's pass is the final guard).
// An empty way holds a code of another cluster (0, or E of cluster 0: no key
// value is reserved). The prologue is two launches, sample and selection:
// the selection zeroes the counters it read and the control words for the
// next join, and the host launches k_hot_clear only when the state is not
// known to be clean (the first join, a failed join, a new buffer or another
// cluster count, a join whose selection did not run). The table is written by
// k_hot_select in every join; the representatives are not cleared (a counter
// that counts in this join was written in this join): nothing else is kept
// from the join before, and nothing relies on what an allocation holds.
#pragma once

#include "phj_partition.h"

namespace phj {

constexpr uint32_t kHotTile = 4096;        // keys of one sample tile
constexpr uint32_t kHotTiles = 128;        // sample tiles, spread evenly over S
constexpr uint32_t kHotTilesPerWg = 4;     // sample tiles of one workgroup of k_hot_sample
constexpr uint32_t kHotCounters = 65536;   // sample counters (L2-resident, 256 KB), 16 bits each in the workgroups' LDS
constexpr uint32_t kHotThreshold = 16;     // sample count of a hot code at kHotTiles tiles (3.1e-5 of S)
constexpr uint32_t kHotHeavy = 8;          // codes sampled this many thresholds over are entered first
constexpr uint32_t kHotBlock = 1024;
constexpr uint32_t kHotStageCount = 4;     // auto mode: a workgroup's counter stands out at this count per tile counted (4 of 4096 keys; uniform keys: none does)
constexpr uint32_t kHotCtlVotes = 4, kHotCtlWords = 8;   // hot_ctl beyond kHotCtl*: 2-3 = the tuples S's pass wrote, 4 = the sample workgroups that flushed
constexpr uint32_t kHotListHeavy = 4096, kHotListRest = 12288;   // k_hot_select's LDS lists of counters at or above the threshold

// dynamic LDS of k_hot_select
__host__ __device__ constexpr size_t hot_select_lds_bytes(uint32_t nb) {
    return static_cast<size_t>(nb) * kHotPer * 8 + static_cast<size_t>(kHotListHeavy + kHotListRest) * 4;
}
static_assert(kHotTilesPerWg * kHotTile <= 65535, "k_hot_sample: the 16-bit halves of an LDS word must not carry");
static_assert(kHotCounters % (4 * kHotBlock) == 0, "k_hot_select: whole 16-B loads of counters per thread");

struct HotArgs {
    const int64_t* rel;     // S: {id, payload} pairs (k_hot_sample COLS: its key column)
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
    unsigned long long* rep;    // [kHotCounters] a code that counted into the counter in this join
    uint32_t staged;        // 1: auto mode, a sample workgroup flushes only if its own counters show skew; 0: it always does
};

// device words of the state: counters, codes, weights, control words, representatives
__host__ __device__ constexpr size_t hot_state_bytes(uint32_t nb) {
    return static_cast<size_t>(kHotCounters) * 4 + static_cast<size_t>(nb) * kHotPer * 16 + kHotCtlWords * 4 +
           static_cast<size_t>(kHotCounters) * 8;
}

__device__ __forceinline__ uint32_t hot_counter_of(uint64_t code) {
    return static_cast<uint32_t>((code * 0x9E3779B97F4A7C15ull) >> 48);
}

// sample tile i of nsamp -> tile of S
__device__ __forceinline__ uint32_t hot_tile_of(const HotArgs& a, uint32_t i) {
    return static_cast<uint32_t>(static_cast<uint64_t>(i) * a.ntiles / a.nsamp);
}

// Counters and control words zeroed: only when the state is not known to be
// clean (k_hot_select leaves it clean for the next join).
__global__ __launch_bounds__(kHotBlock) void k_hot_clear(HotArgs a) {
    const uint32_t i0 = blockIdx.x * kHotBlock + threadIdx.x, step = gridDim.x * kHotBlock;
    for (uint32_t i = i0; i < kHotCounters; i += step) a.counters[i] = 0;
    if (i0 < kHotCtlWords) a.ctl[i0] = 0;
}

// Sample tiles counted in LDS (two 16-bit counters per word: a workgroup
// counts at most kHotTilesPerWg * 4096 keys, so no half carries), kHotTilesPerWg
// per workgroup. Auto mode (a.staged): the keys of the counters that stand out
// (kHotStageCount per tile counted) are added up, and unless they are a
// sixteenth of the keys counted the workgroup returns with nothing written.
// Else every sampled lane leaves its code in its counter's representative
// word, the non-zero counters are added to the global ones (the same number
// of atomic instructions however many tiles were counted) and the workgroup
// votes. No workgroup waits for another: the selection is the next launch.
// COLS: a.rel is the probe side's key column (a relation bound as columns).
template <int HK, bool COLS = false>
__global__ __launch_bounds__(kHotBlock) void k_hot_sample(HotArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t hot_lds[];   // [kHotCounters / 2]
    __shared__ uint32_t sum;
    const uint32_t tid = threadIdx.x;
    const uint32_t b = blockIdx.x;
    const uint32_t s0 = b * kHotTilesPerWg;
    const uint32_t s1 = min(s0 + kHotTilesPerWg, a.nsamp);
    if (s0 >= a.nsamp) return;
    for (uint32_t i = tid; i < kHotCounters / 2; i += kHotBlock) hot_lds[i] = 0;
    if (tid == 0) sum = 0;
    __syncthreads();
    const longlong2* rel = reinterpret_cast<const longlong2*>(a.rel);
    // every key of the workgroup's tiles requested before the first is used
    constexpr uint32_t I = kHotTile / kHotBlock, K = kHotTilesPerWg * I;
    int64_t key[K];   // the keys, then their codes
    uint32_t have = 0;
#pragma unroll
    for (uint32_t k = 0; k < K; k++) {
        const uint32_t si = s0 + k / I;
        const uint32_t ix = hot_tile_of(a, si < s1 ? si : s0) * kHotTile + (k % I) * kHotBlock + tid;
        const bool ok = si < s1 && ix < a.n;
        if constexpr (COLS) key[k] = a.rel[ok ? ix : 0];
        else key[k] = rel[ok ? ix : 0].x;
        have |= (ok ? 1u : 0u) << k;
    }
#pragma unroll
    for (uint32_t k = 0; k < K; k++) {
        if (!((have >> k) & 1u)) continue;
        const uint64_t code = hash64<HK>(static_cast<uint64_t>(key[k]), a.f.seed);
        const uint32_t ci = hot_counter_of(code);
        atomicAdd(&hot_lds[ci >> 1], 1u << ((ci & 1u) * 16));
        key[k] = static_cast<int64_t>(code);
    }
    __syncthreads();
    if (a.staged) {   // workgroup-uniform
        const uint32_t out = kHotStageCount * (s1 - s0);
        uint32_t m = 0;
        for (uint32_t i = tid; i < kHotCounters / 2; i += kHotBlock) {
            const uint32_t v = hot_lds[i], c0 = v & 0xffffu, c1 = v >> 16;
            m += (c0 >= out ? c0 : 0u) + (c1 >= out ? c1 : 0u);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m += __shfl_xor(m, o, 64);
        if ((tid & 63) == 0 && m) atomicAdd(&sum, m);
        __syncthreads();
        const uint64_t cap = static_cast<uint64_t>(s1 - s0) * kHotTile, keys = a.n < cap ? a.n : cap;
        if (static_cast<uint64_t>(sum) * 16 < keys) return;   // no skew here: no global trace
    }
#pragma unroll
    for (uint32_t k = 0; k < K; k++)
        if ((have >> k) & 1u) a.rep[hot_counter_of(static_cast<uint64_t>(key[k]))] = static_cast<unsigned long long>(key[k]);
    for (uint32_t i = tid; i < kHotCounters / 2; i += kHotBlock) {
        const uint32_t v = hot_lds[i];
        if (v & 0xffffu) atomicAdd(&a.counters[2 * i], v & 0xffffu);
        if (v >> 16) atomicAdd(&a.counters[2 * i + 1], v >> 16);
    }
    if (tid == 0) atomicAdd(&a.ctl[kHotCtlVotes], 1u);
}

// The selection, one workgroup: the counters read with coalesced loads, and
// the representative of every counter that reached the
// threshold enters a set of its digit in an LDS copy of the table. The ways
// are tried in fixed order with a 64-bit LDS compare-and-swap and never change
// once taken; a set that is full drops the code. The heavy counters go first
// (a barrier between the rounds), so an overflowing set keeps the larger
// counts. A counter has one representative and a code has one counter, so no
// code is offered twice. The lists hold four times the ways of the largest
// table; a counter past their end is dropped as a full set would drop it. Then the table, zero weights and {entries, sampled
// keys the entries' counters cover} are written out; without a vote from the
// sample that is an empty table at once (nothing was flushed). What the
// sample wrote is zeroed again for the next join: the counters (when there
// was a vote; they are read until the last round) and every control word.
__global__ __launch_bounds__(kHotBlock) void k_hot_select(HotArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long hot_tab[];   // [nb][kHotPer], then the lists
    __shared__ uint32_t s_entries, s_mass, s_scan[kHotBlock / 64];
    const uint32_t tid = threadIdx.x, slots = a.nb * kHotPer;
    uint32_t* hot_list = reinterpret_cast<uint32_t*>(hot_tab + slots);   // [kHotListHeavy + kHotListRest]
    const uint32_t votes = __hip_atomic_load(&a.ctl[kHotCtlVotes], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (uint32_t i = tid; i < slots; i += kHotBlock) hot_tab[i] = i < kHotPer ? a.e0 : 0ull;
    if (tid == 0) s_entries = s_mass = 0;
    __syncthreads();
    if (votes != 0) {   // workgroup-uniform
        // the counters that reached the threshold, compacted into two LDS
        // lists (heavy, the rest: a scan of the threads' numbers of each), so
        // that the rounds below share them evenly: {counter, count} in 16
        // bits each (a count that does not fit is read again)
        constexpr uint32_t V = kHotCounters / (4 * kHotBlock);
        const uint32_t heavy = a.thr * kHotHeavy;
        uint4 cnt[V];
#pragma unroll
        for (uint32_t j = 0; j < V; j++) cnt[j] = reinterpret_cast<const uint4*>(a.counters)[j * kHotBlock + tid];
        uint32_t at[2] = {0, 0};
#pragma unroll
        for (uint32_t j = 0; j < V; j++) {
            const uint32_t c4[4] = {cnt[j].x, cnt[j].y, cnt[j].z, cnt[j].w};
#pragma unroll
            for (uint32_t k = 0; k < 4; k++) {
                at[0] += c4[k] >= heavy ? 1u : 0u;
                at[1] += c4[k] >= a.thr && c4[k] < heavy ? 1u : 0u;
            }
        }
        uint32_t total[2];
        at[0] = block_exclusive_scan_t<kHotBlock / 64>(at[0], s_scan, total[0]);
        at[1] = block_exclusive_scan_t<kHotBlock / 64>(at[1], s_scan, total[1]);
#pragma unroll
        for (uint32_t j = 0; j < V; j++) {
            const uint32_t c4[4] = {cnt[j].x, cnt[j].y, cnt[j].z, cnt[j].w};
#pragma unroll
            for (uint32_t k = 0; k < 4; k++) {
                const uint32_t n = c4[k], item = ((j * kHotBlock + tid) * 4 + k) | (min(n, 0xffffu) << 16);
                if (n >= heavy) {
                    if (at[0] < kHotListHeavy) hot_list[at[0]] = item;
                    at[0]++;
                } else if (n >= a.thr) {
                    if (at[1] < kHotListRest) hot_list[kHotListHeavy + at[1]] = item;
                    at[1]++;
                }
            }
        }
        __syncthreads();
        uint32_t entries = 0, mass = 0;
        for (int round = 0; round < 2; round++) {
            const uint32_t base = round == 0 ? 0u : kHotListHeavy;
            const uint32_t len = min(total[round], round == 0 ? kHotListHeavy : kHotListRest);
            for (uint32_t i = tid; i < len; i += kHotBlock) {
                const uint32_t item = hot_list[base + i], ci = item & 0xffffu;
                const uint32_t n = (item >> 16) == 0xffffu ? a.counters[ci] : item >> 16;
                const unsigned long long code = a.rep[ci];
                const uint32_t d = static_cast<uint32_t>(q_from_hash(code, a.f) >> a.f.shift) & a.f.dmask;
                if (d >= a.nb) continue;
                const unsigned long long empty = d == 0 ? a.e0 : 0ull;
                unsigned long long* set = hot_tab + static_cast<size_t>(d) * kHotPer + (code >> 63) * kHotWays;
                for (uint32_t w = 0; w < kHotWays; w++) {
                    const unsigned long long v = atomicCAS(&set[w], empty, code);
                    if (v == empty) entries++;   // this lane entered it
                    if (v == empty || v == code) {
                        mass += n;
                        break;
                    }
                }
            }
            __syncthreads();
        }
        if (entries) atomicAdd(&s_entries, entries);
        if (mass) atomicAdd(&s_mass, mass);
        __syncthreads();
#pragma unroll
        for (uint32_t j = 0; j < V; j++) reinterpret_cast<uint4*>(a.counters)[j * kHotBlock + tid] = make_uint4(0, 0, 0, 0);
    }
    for (uint32_t i = tid; i < slots; i += kHotBlock) {
        a.code[i] = hot_tab[i];
        a.w[i] = 0;
    }
    // (every thread has read the votes: the barrier after the table's clearing)
    if (tid < kHotCtlWords) a.ctl[tid] = tid == kHotCtlEntries ? s_entries : tid == kHotCtlMass ? s_mass : 0u;
}

}  // namespace phj
