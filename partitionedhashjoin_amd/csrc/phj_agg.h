// phj_agg.h — aggregates over the join without its rows, for gfx950:
// phj_join_aggregate's totals (pairs, probe tuples with a partner, Σ build
// payload, Σ probe payload, Σ of their product over R ⋈ S) and, per build
// tuple, its number of probe partners and the sum of their payloads.
//
// One pass over the join the inner join's count pass does (phj_inner.h), with
// nothing stored per pair and nothing addressed per pair, so there is no
// limit at 2^32 pairs. Every sum is unsigned 64-bit arithmetic (modulo 2^64):
// it does not depend on the order of the additions, so the results are exact
// whatever the schedule of the atomics.
//   totals: per probe key, n = equal build keys and A = Σ of their payloads;
//           the lane adds n, A, n * pb, A * pb in registers; one block
//           reduction and one global atomic per total per workgroup.
//   groups: one accumulator pair per element of the build storage (the hit
//           flags' indexing, phj_outer.h: rows of the partitioned build
//           relation, or bucket slots), two planes of 64-bit words:
//           acc[i] = partners, acc[nF + i] = Σ probe payload; cleared by the
//           host before the launch, compacted into phj_group_row's afterwards
//           (k_build_only_count / k_build_only_write's scheme).
// The kernels take k_inner_fused's and k_np_inner's structure, not their
// symbols: those instantiations' generated code stays as it is.
#pragma once

#include "phj_outer.h"

namespace phj {

struct GroupRow {   // == phj_group_row
    int64_t id, payload_a;
    uint64_t partners;
    int64_t sum_b;
};

constexpr int kAggTotals = 5;   // {pairs, probe_matched, sum_a, sum_b, sum_ab}: the order of phj_join_totals

// The workgroup's five totals into res[0, 5): one atomic per non-zero total.
__device__ __forceinline__ void agg_block_totals(const unsigned long long (&v)[kAggTotals],
                                                 unsigned long long (&red)[kAggTotals][kWaves],
                                                 unsigned long long* res) {
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < kAggTotals; k++) {
        const unsigned long long x = wave_sum(v[k]);
        if (lane == 0) red[k][wave] = x;
    }
    __syncthreads();
    if (threadIdx.x < kAggTotals) {
        unsigned long long t = 0;
        for (int w = 0; w < kWaves; w++) t += red[threadIdx.x][w];
        if (t) atomicAdd(res + threadIdx.x, t);
    }
}

// Radix form: k_inner_fused's work split (one wave per (partition, S chunk)
// item, the partition's build keys in the wave's LDS CSR table in rounds of
// 256, every probe key compared with its whole bucket in every round). The
// build payloads are staged in LDS beside the keys at the scatter step (a hit
// needs one, and the gather rpays[row] per hit is then an LDS read).
// "Some round matched" is one bit per probe key of the item: an item holds
// exactly 64 keys per lane (16 sub-rounds x 4), so one 64-bit register per
// lane carries it across the rounds.
// A bucket of kInnerWide keys or more is compared by the whole wave (the count
// pass's rule for when lane by lane is cheaper); each lane adds its share of
// that key's n and A to its own totals, so nothing is reduced over the wave.
// GROUPS: two LDS accumulators per build tuple of the round, indexed by the
// tuple's in-round index f (kept beside the key in lf[], as BMARK keeps it in
// lr[]): partners (32 bits: an item has at most 4096 probe keys) and Σ probe
// payload, cleared per round. After the round's probe loop lane f adds its
// non-zero pair to the global planes at rlo + r0 + f: 64 consecutive 8-B
// words per instruction; atomics, because several items serve one partition.
template <int HK, bool GROUPS>
__global__ __launch_bounds__(kBlock) void k_agg_fused(FusedArgs a, const int64_t* spays, unsigned long long* res,
                                                      unsigned long long* acc, uint64_t nF) {
    constexpr int TCAP = 256, RPL = TCAP / 64, OCAP = TCAP / 2 + 1, KPL = 4;
    constexpr uint32_t SUB = 64 * KPL;
    static_assert(kFusedChunk / SUB * KPL == 64, "one matched bit per probe key of an item in a 64-bit register");
    constexpr int GCAP = GROUPS ? TCAP : 1;
    __shared__ int64_t lk_all[kWaves][TCAP];
    __shared__ int64_t lp_all[kWaves][TCAP];
    __shared__ uint32_t lo_all[kWaves][OCAP];
    __shared__ uint32_t cur_all[kWaves][OCAP];
    __shared__ uint32_t lf_all[kWaves][GCAP];
    __shared__ uint32_t gn_all[kWaves][GCAP];
    __shared__ unsigned long long gs_all[kWaves][GCAP];
    __shared__ unsigned long long red[kAggTotals][kWaves];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int64_t* lk = lk_all[wave];
    int64_t* lp = lp_all[wave];
    uint32_t* loffs = lo_all[wave];
    uint32_t* lcur = cur_all[wave];
    uint32_t* lf = lf_all[wave];
    uint32_t* gn = gn_all[wave];
    unsigned long long* gs = gs_all[wave];
    const int64_t* rkeys = a.L.seg[0].keys;
    const int64_t* rpays = a.L.seg[0].pays;
    const uint32_t* rb = a.L.seg[0].bounds;
    unsigned long long tot[kAggTotals] = {0, 0, 0, 0, 0};
    for (uint32_t item = blockIdx.x * kWaves + wave; item < a.nitems; item += gridDim.x * kWaves) {
        const FusedItem it = a.items[item];
        if (it.s_cnt == 0) continue;
        const uint32_t rlo = rb[it.p], m = rb[it.p + 1] - rlo;
        if (m == 0) continue;   // no build tuple: no pair, no group
        const uint32_t nsub = (it.s_cnt + SUB - 1) / SUB;
        uint64_t matched = 0;   // bit (sub * KPL + j): that probe key of this lane met an equal build key
        for (uint32_t r0 = 0; r0 < m; r0 += TCAP) {
            const uint32_t mr = min(static_cast<uint32_t>(TCAP), m - r0);
            const uint32_t nbk = table_buckets(mr);
            int64_t rk[RPL], rp[RPL];
            uint32_t bk[RPL];
#pragma unroll
            for (int j = 0; j < RPL; j++) {
                const uint32_t f = j * 64 + lane;
                rk[j] = f < mr ? rkeys[rlo + r0 + f] : 0;
                rp[j] = f < mr ? rpays[rlo + r0 + f] : 0;
            }
            for (uint32_t i = lane; i < nbk; i += 64) lcur[i] = 0;
            if (GROUPS) {
#pragma unroll
                for (int j = 0; j < RPL; j++) {
                    gn[j * 64 + lane] = 0;
                    gs[j * 64 + lane] = 0;
                }
            }
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
                const uint32_t x = wave_scan_incl(v, lane);
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
                    lp[pos] = rp[j];
                    if (GROUPS) lf[pos] = f;
                }
            }
            wave_lds_sync();
            for (uint32_t sub = 0; sub < nsub; sub++) {
#pragma unroll
                for (int j = 0; j < KPL; j++) {
                    const uint32_t off = sub * SUB + j * 64 + lane;
                    const bool act = off < it.s_cnt;
                    const uint32_t s = it.s_lo + (act ? off : 0u);
                    const int64_t key = act ? a.skeys[s] : 0;
                    const unsigned long long pb = act ? static_cast<unsigned long long>(spays[s]) : 0ull;
                    const uint32_t b = bucket_of(hash64<HK>(static_cast<uint64_t>(key), a.seed), nbk);
                    const uint32_t t0 = act ? loffs[b] : 0u, t1 = act ? loffs[b + 1] : 0u;
                    // (every lane of the wave gets here: the item and round loops are per wave)
                    uint64_t todo = __ballot(t1 - t0 >= kInnerWide);
                    if (__popcll(todo) > static_cast<int>(kInnerWideLanes)) todo = 0;
                    const bool wide = (todo >> lane) & 1;
                    unsigned long long n = 0, A = 0;
                    bool wide_hit = false;
                    if (!wide) {
                        for (uint32_t t = t0; t < t1; t++) {
                            if (lk[t] == key) {
                                n++;
                                A += static_cast<unsigned long long>(lp[t]);
                                if (GROUPS) {   // (lanes on one hot probe key add to the same words)
                                    const uint32_t f = lf[t];
                                    atomicAdd(&gn[f], 1u);
                                    atomicAdd(&gs[f], pb);
                                }
                            }
                        }
                    }
                    while (todo) {
                        const int src = __ffsll(static_cast<unsigned long long>(todo)) - 1;
                        todo &= todo - 1;
                        const int64_t wkey = __shfl(key, src, 64);
                        const uint32_t w1 = __shfl(t1, src, 64);
                        const unsigned long long wpb = __shfl(pb, src, 64);
                        // the totals are sums over every lane anyway: each lane keeps
                        // its own share of this key's n and A (no reduction over the
                        // wave); only "matched" goes back to the key's lane
                        unsigned long long wn = 0, wA = 0;
                        for (uint32_t base = __shfl(t0, src, 64); base < w1; base += 64) {
                            const uint32_t t = base + lane;
                            const bool hit = t < w1 && lk[t] == wkey;
                            if (hit) {   // every lane its own t: no two lanes on one word
                                wn++;
                                wA += static_cast<unsigned long long>(lp[t]);
                                if (GROUPS) {
                                    const uint32_t f = lf[t];
                                    atomicAdd(&gn[f], 1u);
                                    atomicAdd(&gs[f], wpb);
                                }
                            }
                        }
                        tot[0] += wn;
                        tot[2] += wA;
                        tot[3] += wn * wpb;
                        tot[4] += wA * wpb;
                        const bool any = __ballot(wn != 0) != 0;
                        if (any && lane == static_cast<uint32_t>(src)) wide_hit = true;
                    }
                    tot[0] += n;
                    tot[2] += A;
                    tot[3] += n * pb;
                    tot[4] += A * pb;
                    if (n || wide_hit) matched |= 1ull << (sub * KPL + j);
                }
            }
            if (GROUPS) {
                wave_lds_sync();   // every lane's adds before they are read
#pragma unroll
                for (int j = 0; j < RPL; j++) {
                    const uint32_t f = j * 64 + lane;
                    const uint32_t pn = f < mr ? gn[f] : 0u;
                    if (pn) {
                        const uint64_t e = static_cast<uint64_t>(rlo) + r0 + f;
                        if (e < nF) {
                            atomicAdd(acc + e, static_cast<unsigned long long>(pn));
                            atomicAdd(acc + nF + e, gs[f]);
                        }
                    }
                }
            }
            wave_lds_sync();   // this round's LDS reads before the next round's stores
        }
        tot[1] += __popcll(matched);
    }
    agg_block_totals(tot, red, res);
}

// NoPartitioning form on k_np_inner's walk: from the home bucket through the
// run of full buckets, wrapping at the table's end, at most nb buckets; n and
// A per probe tuple in registers, A from pays[b * kNPSlots + s].
// GROUPS: global atomics into the planes at b * kNPSlots + s. The lanes of a
// wave with the same key are merged first (a hot probe key: a few per cent of
// S on one slot): every lane offers its lane number in a 128-entry LDS table
// at its home bucket's low bits; a lane that reads another lane there with
// its own key adds {1, pb} to that lane's LDS pair and leaves the walk to it.
// The winner of an entry reads itself, so it always walks; lanes of other keys
// on the same entry are simply not merged. A walking lane stands for c probe
// tuples with payload sum sb: its totals are n * c, A * c, n * sb, A * sb.
template <int HK, bool GROUPS>
__global__ __launch_bounds__(kBlock) void k_np_agg(const longlong2* S, uint64_t nS, const NPBucket* tab,
                                                   const int64_t* pays, NPHome g, uint64_t seed,
                                                   unsigned long long* res, unsigned long long* acc, uint64_t nF) {
    constexpr int IT = 4;   // as k_np_probe: every home bucket of a round requested before any compare
    constexpr int MCAP = GROUPS ? 64 : 1;
    __shared__ unsigned long long red[kAggTotals][kWaves];
    __shared__ uint32_t win_all[kWaves][2 * MCAP];
    __shared__ int64_t mk_all[kWaves][MCAP];
    __shared__ uint32_t mc_all[kWaves][MCAP];
    __shared__ unsigned long long ms_all[kWaves][MCAP];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint32_t* win = win_all[wave];
    int64_t* mk = mk_all[wave];
    uint32_t* mc = mc_all[wave];
    unsigned long long* ms = ms_all[wave];
    unsigned long long tot[kAggTotals] = {0, 0, 0, 0, 0};
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kBlock * IT;
    // (the trip count is the same for every thread of the workgroup: base does not depend on threadIdx)
    for (uint64_t base = static_cast<uint64_t>(blockIdx.x) * kBlock * IT; base < nS; base += stride) {
        longlong2 t[IT];
        uint32_t b[IT];
        longlong2 q[IT][4];
        np_probe_front<HK, true>(S, nS, base, tab, g, seed, t, b, q);
#pragma unroll
        for (int j = 0; j < IT; j++) {
            const uint64_t i = base + static_cast<uint64_t>(j) * kBlock + threadIdx.x;
            const bool act = i < nS;
            const int64_t key = t[j].x;
            unsigned long long c = 1, sb = static_cast<unsigned long long>(t[j].y);
            bool walk = act;
            if (GROUPS) {
                const uint32_t e = b[j] & (2 * MCAP - 1);
                mk[lane] = key;
                mc[lane] = 1;
                ms[lane] = sb;
                if (act) win[e] = lane;
                wave_lds_sync();
                const uint32_t w = act ? win[e] : lane;
                const bool dup = w != lane && mk[w] == key;
                if (dup) {
                    atomicAdd(&mc[w], 1u);
                    atomicAdd(&ms[w], sb);
                    walk = false;
                }
                wave_lds_sync();
                c = mc[lane];
                sb = ms[lane];
                wave_lds_sync();   // read before the next round's stores
            }
            if (!walk) continue;
            unsigned long long n = 0, A = 0;
            uint32_t bb = b[j];
            longlong2 w[4];
#pragma unroll
            for (int x = 0; x < 4; x++) w[x] = q[j][x];
            for (uint32_t step = 0;;) {
                int64_t ks[kNPSlots];
                const uint32_t fill = np_unpack(w, ks);
                const uint32_t cs = fill < kNPSlots ? fill : kNPSlots;
#pragma unroll
                for (int s = 0; s < kNPSlots; s++) {
                    if (static_cast<uint32_t>(s) < cs && ks[s] == key) {
                        const uint64_t e = static_cast<uint64_t>(bb) * kNPSlots + s;
                        n++;
                        A += static_cast<unsigned long long>(pays[e]);
                        if (GROUPS && e < nF) {
                            atomicAdd(acc + e, c);
                            atomicAdd(acc + nF + e, sb);
                        }
                    }
                }
                if (fill < kNPSlots || ++step >= g.nb) break;   // full bucket: the run goes on
                bb = (bb + 1 == g.nb) ? 0 : bb + 1;
                const longlong2* bp = reinterpret_cast<const longlong2*>(tab + bb);
#pragma unroll
                for (int x = 0; x < 4; x++) w[x] = bp[x];
            }
            tot[0] += n * c;
            tot[1] += n ? c : 0ull;
            tot[2] += A * c;
            tot[3] += n * sb;
            tot[4] += A * sb;
        }
    }
    agg_block_totals(tot, red, res);
}

// Element i of the build storage holds a build tuple whose group row is kept.
// NP: the storage is the bucket table's slots, of which s < min(fill,
// kNPSlots) hold a tuple (build_unhit's rule); matched: only with a partner.
template <bool NP>
__device__ __forceinline__ bool group_kept(uint64_t i, uint64_t n, const unsigned long long* acc, const NPBucket* tab,
                                           bool matched) {
    if (i >= n) return false;
    if (NP) {
        const uint32_t b = static_cast<uint32_t>(i / kNPSlots), s = static_cast<uint32_t>(i % kNPSlots);
        if (s >= tab[b].fill) return false;   // (fill > kNPSlots once full: s < kNPSlots always)
    }
    return !matched || acc[i] != 0;
}

// Kept group rows per compaction block -> cnt[block] (cnt has nblocks + 1
// entries; the exclusive scan turns it into row offsets), *count += their sum.
template <bool NP>
__global__ __launch_bounds__(kBlock) void k_agg_group_count(const unsigned long long* acc, const NPBucket* tab,
                                                            uint64_t n, bool matched, uint32_t* cnt,
                                                            unsigned long long* count) {
    __shared__ uint32_t red[kWaves];
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kMatBlock;
    uint32_t c = 0;
#pragma unroll
    for (uint32_t j = 0; j < kMatBlockItems; j++)
        c += group_kept<NP>(base + j * kBlock + threadIdx.x, n, acc, tab, matched) ? 1u : 0u;
    c = block_sum(c, red);
    if (threadIdx.x == 0) {
        cnt[blockIdx.x] = c;
        if (c) atomicAdd(count, static_cast<unsigned long long>(c));
    }
}

// The group rows of one compaction block's kept elements from
// out[offs[block]] on (k_build_only_write's positions). NP: keys from the
// table's slots, payloads pays[i]; else keys[i], pays[i]. Rows from nrows on
// are not stored (the count kernel saw the same planes: there are none).
template <bool NP>
__global__ __launch_bounds__(kBlock) void k_agg_group_write(const unsigned long long* acc, const NPBucket* tab,
                                                            uint64_t n, bool matched, const int64_t* keys,
                                                            const int64_t* pays, const uint32_t* offs, GroupRow* out,
                                                            uint64_t nrows) {
    __shared__ uint32_t wcnt[kWaves];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kMatBlock;
    uint64_t row = offs[blockIdx.x];
    for (uint32_t j = 0; j < kMatBlockItems; j++) {
        const uint64_t i = base + j * kBlock + threadIdx.x;
        const bool keep = group_kept<NP>(i, n, acc, tab, matched);
        const uint64_t bal = __ballot(keep);
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
        const uint64_t at = row + wbase + before;
        if (keep && at < nrows) {
            GroupRow r;
            r.id = NP ? tab[i / kNPSlots].key[i % kNPSlots] : keys[i];
            r.payload_a = pays[i];
            r.partners = acc[i];
            r.sum_b = static_cast<int64_t>(acc[n + i]);
            out[at] = r;
        }
        row += total;
        __syncthreads();   // wcnt reused by the next round
    }
}

// An empty probe side: build tuple i's group row {id, payload, 0, 0} at out[i].
__global__ __launch_bounds__(kBlock) void k_agg_group_side(const longlong2* rel, uint64_t n, GroupRow* out) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kBlock;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride) {
        const longlong2 t = rel[i];
        GroupRow r;
        r.id = t.x;
        r.payload_a = t.y;
        r.partners = 0;
        r.sum_b = 0;
        out[i] = r;
    }
}

}  // namespace phj
