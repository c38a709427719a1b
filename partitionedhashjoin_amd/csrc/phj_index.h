// phj_index.h — row-number joins for gfx950: what is only phj_join_indices'
// and phj_gather_column's.
//
// phj_join_indices is phj_join_rows with two changes at the ends of the same
// passes (DESIGN.md §3 "Row-number joins"):
//   - pass 1 (phj_partition.h load_key_row: k_scatter, k_scatter_chunked, and
//     k_hist's key-column read) and the NoPartitioning probe (phj_inner.h
//     np_probe_front_keys) read keys alone, a key column or the tuples' ids,
//     and take the tuple's position in the bound relation as its payload;
//     everything between carries that number as the payload it already carries;
//   - every kernel that writes a row stores into an IndexSink (phj_inner.h):
//     build_rows[at] and probe_rows[at], 16 B per row, PHJ_NO_ROW for the
//     missing side.
// The caller gathers as many columns as it has with the two index columns:
// torch's index_select, or k_gather_column below.
#pragma once

#include "phj_outer.h"

namespace phj {

constexpr int64_t kNoRow = -1;   // == PHJ_NO_ROW

// out[i] = src[idx[i]] for idx[i] in [0, src_n). Every other index is never
// dereferenced: out[i] = null_value, or (KEEP: the caller passed no null value)
// out[i] stays as it is, so a second gather into the same column fills what
// the first left. Indices other than kNoRow outside the range are counted into
// *bad, summed over the wave first: a column of bad indices costs one atomic
// per wave. Grid-stride over i: the index loads and the stores are coalesced
// (512 B per wave), the loads of src are the gather.
template <bool KEEP>
__global__ __launch_bounds__(kBlock) void k_gather_column(const int64_t* src, uint64_t src_n, const int64_t* idx,
                                                          uint64_t n, int64_t null_value, int64_t* out,
                                                          unsigned long long* bad) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kBlock;
    unsigned long long nbad = 0;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride) {
        const int64_t j = __builtin_nontemporal_load(idx + i);
        if (static_cast<uint64_t>(j) < src_n) {
            out[i] = src[j];
        } else {
            if (!KEEP) out[i] = null_value;
            nbad += j != kNoRow ? 1u : 0u;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nbad += __shfl_down(nbad, o, 64);
    if ((threadIdx.x & 63) == 0 && nbad) atomicAdd(bad, nbad);
}

}  // namespace phj
