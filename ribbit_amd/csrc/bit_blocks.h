// bit_blocks.h -- a bitmap of one bit per base read in blocks of LOCI_LANE_WORDS words, as overlap.hip and composition.hip read
// the coverage bitmaps and the bit planes: the 16-byte loads of a block, and the ones before a position within its block, which
// a caller adds to the block's entry of an exclusive scan of the blocks' counts to get a prefix count at the position.
// Device code only; included by .hip files.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace rb {

static_assert(LOCI_LANE_WORDS == 8, "a lane loads a block's words as two dwordx4");

// the words of block t; `words` is 16-byte aligned and padded to whole blocks
__device__ inline void load_block(const uint32_t *__restrict__ words, int64_t t, uint32_t (&w)[LOCI_LANE_WORDS]) {
    const uint4 a = *(const uint4 *)(words + LOCI_LANE_WORDS * t), b = *(const uint4 *)(words + LOCI_LANE_WORDS * t + 4);
    w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
    w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
}

// the block of position p, and the mask of the bits below p in p's word
__device__ inline int64_t block_of(int64_t p) { return (p >> 5) / LOCI_LANE_WORDS; }
__device__ inline uint32_t bits_below(int64_t p) { return (1u << (p & 31)) - 1u; }

// set bits at the positions of p's block before p: the whole words before p's word (at most 7) and p's word below p
__device__ inline uint32_t ones_before_in_block(const uint32_t *__restrict__ bits, int64_t p) {
    const int64_t w = p >> 5;
    uint32_t r = 0;
    for (int64_t j = block_of(p) * LOCI_LANE_WORDS; j < w; ++j) r += (uint32_t)__popc(bits[j]);
    return r + (uint32_t)__popc(bits[w] & bits_below(p));
}

}  // namespace rb
