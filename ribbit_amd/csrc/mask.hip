// mask.hip -- the repeat mask of a loaded record (api_mask.cpp: ribbit_hip_mask_record).  Two kernels on the handle's stream:
//   coverage: the BED rows' half-open intervals -> a 1-bit-per-base bitmap (L/32 + 1 words, zeroed beforehand)
//   format:   bases + bitmap -> the masked body in lines of W bases, each ending in '\n', 16 output bytes per thread
// Both are HBM-bound: the format kernel reads 1 byte and 1/8 bit-byte per base and writes 1 + 1/W bytes.
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace rb {

namespace {

constexpr int MASK_THREADS = 256;
constexpr int64_t MASK_MAX_BLOCKS = 256 * 32;      // blocks of a launch at most; the kernels stride
// interior words a lane sets on its own; longer intervals are set by the whole wave, 64 words per store instruction
constexpr int32_t MASK_LANE_WORDS = 8;

// One lane per interval, intervals in grid-stride waves.  The two boundary words of an interval are OR-ed atomically
// (another interval may share them); the words between are all ones and stored plainly (the same value, whatever the
// order).  An interval longer than MASK_LANE_WORDS words is spread over its wave: the wave walks its lanes' long
// intervals one after the other, each with all 64 lanes.  Every interval is clipped to [0, length) before an address
// is formed.
__global__ void __launch_bounds__(MASK_THREADS) mask_coverage_kernel(const int32_t *__restrict__ iv, int64_t n, int64_t length,
                                                                      uint32_t *__restrict__ bits) {
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * (MASK_THREADS / 64);
    for (int64_t base = ((int64_t)blockIdx.x * (MASK_THREADS / 64) + (threadIdx.x >> 6)) * 64; base < n; base += waves * 64) {
        const int64_t i = base + lane;
        int32_t lo = 0, hi = 0;      // interior words [lo, hi) of a long interval
        if (i < n) {
            const int64_t s = max((int64_t)iv[2 * i], (int64_t)0), e = min((int64_t)iv[2 * i + 1], length);
            if (s < e) {
                const int32_t ws = (int32_t)(s >> 5), we = (int32_t)((e - 1) >> 5);
                const uint32_t head = ~0u << (s & 31), tail = ~0u >> (31 - ((e - 1) & 31));
                if (ws == we) {
                    atomicOr(bits + ws, head & tail);
                } else {
                    atomicOr(bits + ws, head);
                    atomicOr(bits + we, tail);
                    if (we - ws - 1 <= MASK_LANE_WORDS) {
                        for (int32_t w = ws + 1; w < we; ++w) bits[w] = ~0u;
                    } else {
                        lo = ws + 1;
                        hi = we;
                    }
                }
            }
        }
        uint64_t longs = __ballot(hi > lo);
        while (longs) {
            const int src = __ffsll((unsigned long long)longs) - 1;
            longs &= longs - 1;
            const int32_t l = __shfl(lo, src), h = __shfl(hi, src);
            for (int32_t w = l + lane; w < h; w += 64) bits[w] = ~0u;
        }
    }
}

// The output byte o of the body is, with P = width + 1: a '\n' when o % P == width or o is the last byte; else the base
// at (o / P) * width + o % P.  A thread makes output bytes [16 c, 16 c + 16): it finds the line and column of the first
// one once (a multiply-high by the host's floor((2^64 - 1) / P), then at most two corrections), loads the 16 bases
// from there as two aligned 16-byte loads (one 128-bit funnel shift brings them to byte 0) and the coverage bits as a
// 64-bit window, then walks the 16 bytes, consuming a base for each byte that is not a line end.  The buffer is padded
// to a multiple of 16 bytes: every thread stores a whole dwordx4 (bytes past the body are 0).
__global__ void __launch_bounds__(MASK_THREADS) mask_format_kernel(const uint8_t *__restrict__ ascii, int64_t length,
                                                                    const uint32_t *__restrict__ bits, int64_t nwords, int hard,
                                                                    int64_t width, uint64_t recip, int64_t out_len,
                                                                    uint4 *__restrict__ out) {
    const int64_t chunks = (out_len + 15) >> 4;
    const uint64_t period = (uint64_t)width + 1;
    for (int64_t c = (int64_t)blockIdx.x * MASK_THREADS + threadIdx.x; c < chunks; c += (int64_t)gridDim.x * MASK_THREADS) {
        const uint64_t o0 = (uint64_t)c << 4;
        uint64_t line = __umul64hi(o0, recip);
        uint64_t col = o0 - line * period;
        if (col >= period) { col -= period; ++line; }
        if (col >= period) { col -= period; ++line; }
        const int64_t i0 = (int64_t)(line * (uint64_t)width + col);      // the first base this chunk consumes
        // bases i0 .. i0 + 15 into (r0, r1), byte 0 first; past the record's end: 0
        uint64_t r0 = 0, r1 = 0;
        const uint8_t *p = ascii + i0;
        const uint8_t *pa = (const uint8_t *)((uintptr_t)p & ~(uintptr_t)15);
        if (i0 < length) {
            if (pa >= ascii && pa + 32 <= ascii + length) {
                const uint4 a = *(const uint4 *)pa, b = *(const uint4 *)(pa + 16);
                uint64_t q0 = (uint64_t)a.y << 32 | a.x, q1 = (uint64_t)a.w << 32 | a.z;
                uint64_t q2 = (uint64_t)b.y << 32 | b.x, q3 = (uint64_t)b.w << 32 | b.z;
                const int off = (int)(p - pa);
                if (off >= 8) { q0 = q1; q1 = q2; q2 = q3; }
                const int sh = (off & 7) * 8;
                r0 = sh ? (q0 >> sh) | (q1 << (64 - sh)) : q0;
                r1 = sh ? (q1 >> sh) | (q2 << (64 - sh)) : q1;
            } else {
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    const uint64_t v = i0 + k < length ? (uint64_t)p[k] : 0;
                    if (k < 8) r0 |= v << (8 * k); else r1 |= v << (8 * (k - 8));
                }
            }
        }
        uint32_t cov = 0;
        if (i0 < length) {
            const int64_t w = i0 >> 5;
            const uint64_t win = (uint64_t)(w + 1 < nwords ? bits[w + 1] : 0) << 32 | bits[w];
            cov = (uint32_t)(win >> (i0 & 31));
        }
        uint64_t lo = 0, hi = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int64_t o = (int64_t)o0 + k;
            uint64_t v;
            if (o >= out_len) {
                v = 0;
            } else if (col == (uint64_t)width || o == out_len - 1) {
                v = '\n';
                col = 0;
            } else {
                const uint32_t ch = (uint32_t)(r0 & 0xff);
                const bool m = cov & 1u;
                v = !m ? ch : hard ? (uint32_t)'N' : (ch - 'A' <= (uint32_t)('Z' - 'A') ? (ch | 0x20u) : ch);
                r0 = (r0 >> 8) | (r1 << 56);
                r1 >>= 8;
                cov >>= 1;
                ++col;
            }
            if (k < 8) lo |= v << (8 * k); else hi |= v << (8 * (k - 8));
        }
        out[c] = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
    }
}

}  // namespace

void launch_mask_coverage(const int32_t *intervals, int64_t n, int64_t length, uint32_t *bits, hipStream_t stream) {
    if (n <= 0) return;
    hipLaunchKernelGGL(mask_coverage_kernel, dim3(grid_for(n, MASK_THREADS, MASK_MAX_BLOCKS)), dim3(MASK_THREADS), 0, stream, intervals, n, length, bits);
}

void launch_mask_format(const uint8_t *ascii, int64_t length, const uint32_t *bits, int64_t nwords, int hard, int64_t width,
                        int64_t out_len, uint8_t *out, hipStream_t stream) {
    if (out_len <= 0) return;
    const uint64_t recip = ~(uint64_t)0 / ((uint64_t)width + 1);
    hipLaunchKernelGGL(mask_format_kernel, dim3(grid_for((out_len + 15) >> 4, MASK_THREADS, MASK_MAX_BLOCKS)), dim3(MASK_THREADS), 0, stream, ascii, length, bits, nwords,
                       hard, width, recip, out_len, (uint4 *)out);
}

}  // namespace rb
