// primers.hip -- a forward primer in the left flank and a reverse primer in the right flank of every target of the loaded record
// (api_primers.cpp: ribbit_hip_record_primers; include/ribbit_hip.h has the contract).  One wavefront per (target, side),
// PRIMER_WAVES of them to a workgroup, each with its own slice of LDS for a window of up to `cap` bases (the flank); the
// wavefronts of a workgroup never wait for each other (no __syncthreads).  The window's staging, expansion, prefix scans and the
// verdict on one candidate are primer_window.h's, shared with primer_pairs.hip; what is here:
//   search:   a lane takes the starts p = lane, lane + 64, ... and every length k for each (judge).  The lane keeps the least key
//             penalty << 32 | distance << 8 | k and counts the admissible ones
//   result:   the wave's least key (__shfl_xor) and the sum of the counts (wave_sum); lane 0 takes start and Tm from the key
//             again and reads the candidate's bases from LDS
// LDS: 3 words and a byte per position, 13.5 KB per wavefront at the largest flank, 54 KB per workgroup: two workgroups fit a
// CU's 160 KB there, and at the default flank of 200 (2.7 KB per wavefront) the wavefronts' registers are what limits them.
// The kernel strides beyond ROW_MAX_BLOCKS blocks.
#include <hip/hip_runtime.h>

#include "primer_window.h"

namespace rb {

namespace {

constexpr int PRIMER_WAVES = 4;
constexpr int PRIMER_THREADS = 64 * PRIMER_WAVES;
static_assert(PRIMER_THREADS == ROW_THREADS, "the launch shape of the row outputs");

__global__ void __launch_bounds__(PRIMER_THREADS) primers_kernel(const int32_t *__restrict__ targets, int64_t n_targets, DevicePlanes pl, const uint32_t *__restrict__ bits,
                                                                RibbitPrimerParams prm, int cap, RibbitRowPrimers *__restrict__ out) {
    extern __shared__ uint32_t lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const Window win = window_at(lds + (size_t)wave * wave_lds_words(cap), cap);
    const int64_t length = pl.length, items = 2 * n_targets;
    const int look_back = run_look_back(prm);
    for (int64_t item = (int64_t)blockIdx.x * PRIMER_WAVES + wave; item < items; item += (int64_t)gridDim.x * PRIMER_WAVES) {
        const int64_t t = item >> 1;
        const bool right = item & 1;
        const int64_t s = min(max((int64_t)targets[2 * t], (int64_t)0), length), e = min(max((int64_t)targets[2 * t + 1], s), length);
        const int64_t from = right ? e : max(s - (int64_t)prm.flank, (int64_t)0), to = right ? min(e + (int64_t)prm.flank, length) : s;
        const int n = (int)(to - from);      // 0 .. flank <= cap
        fill_window(win, cap, pl, bits, from, n, look_back, lane);
        // search
        unsigned long long best = NO_KEY;
        uint32_t found = 0;
        for (int p = lane; p + prm.min_length <= n; p += 64) {
            const uint32_t before = win.cnt[p], first = win.code[p] & 3u;
            for (int k = prm.min_length; k <= prm.max_length && p + k <= n; ++k) {
                int32_t tm;
                const Verdict v = judge(win, prm, right, p, k, before, first, tm);
                if (v == STOP) break;
                if (v == SKIP) continue;
                ++found;
                const unsigned long long key = candidate_key(prm, right, p, k, n, tm);
                best = key < best ? key : best;
            }
        }
        best = wave_min(best);
        const unsigned long long total = wave_sum(found);
        if (lane == 0) {
            RibbitPrimer r{-1, 0, 0, 0, 0, 0};
            if (best != NO_KEY) r = primer_of(win, best, right, from, n);
            if (right) {
                out[t].right = r;
                out[t].right_candidates = (int32_t)total;
            } else {
                out[t].left = r;
                out[t].left_candidates = (int32_t)total;
            }
        }
        wave_sync();      // (the next window is staged over this one)
    }
}

}  // namespace

PrimerLayout primers_layout(int64_t n_targets) {
    PrimerLayout at{};
    WorkCarver w;
    at.out = w.take((size_t)n_targets * sizeof(RibbitRowPrimers));
    w.close(at, 0);
    return at;
}

hipError_t launch_primers(const DevicePlanes &pl, const uint32_t *bits, const int32_t *targets, int64_t n_targets, const RibbitPrimerParams &prm, uint8_t *work,
                          size_t work_bytes, const PrimerLayout &at, hipStream_t stream) {
    if (work_bytes < at.bytes || prm.flank < 0 || prm.flank > RIBBIT_PRIMER_MAX_FLANK || prm.min_length < 2 || prm.max_length > RIBBIT_PRIMER_MAX_LENGTH) return hipErrorInvalidValue;
    const int cap = std::max(prm.flank, 1);
    const size_t lds_bytes = (size_t)PRIMER_WAVES * wave_lds_words(cap) * sizeof(uint32_t);      // 54 KB at most
    hipLaunchKernelGGL(primers_kernel, dim3(grid_for(2 * n_targets, PRIMER_WAVES, ROW_MAX_BLOCKS)), dim3(PRIMER_THREADS), lds_bytes, stream, targets, n_targets, pl,
                       bits, prm, cap, region<RibbitRowPrimers>(work, at.out));
    return hipGetLastError();
}

}  // namespace rb
