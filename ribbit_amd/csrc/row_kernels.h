// row_kernels.h -- what the kernels of the row outputs (overlap.hip, best.hip, classes.hip, compound.hip, interruptions.hip,
// nearest.hip, composition.hip, primers.hip, primer_pairs.hip, primer_products.hip, primer_specific.hip) write the same way: the shape of a launch, a row clipped to the record, a sum over a wavefront, the
// bits a sort key of positions needs.  Included by .hip files only.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace rb {

constexpr int ROW_THREADS = 256;
constexpr int64_t ROW_MAX_BLOCKS = 1024;      // blocks of a launch at most (four per CU); the kernels stride

// row i of iv clipped to [0, length), in 64-bit; empty when s >= e
struct RowSpan { int64_t s, e; };
__host__ __device__ inline RowSpan clip_row(const int32_t *__restrict__ iv, int64_t i, int64_t length) {
    return RowSpan{max((int64_t)iv[2 * i], (int64_t)0), min((int64_t)iv[2 * i + 1], length)};
}

__device__ inline unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d);
    return v;      // (lane 0's)
}

// the least b >= 1 with v < 2^b, at most 32: the bits of a sort key that holds the positions 0 .. v
inline unsigned bits_for(int64_t v) {
    unsigned bits = 1;
    while (bits < 32 && (v >> bits)) ++bits;
    return bits;
}

}  // namespace rb
