// alleles.hip -- every marker's alleles over many samples: the kinds of its cells, the distinct sizes among the typed ones, the
// most frequent size and the numerators of He and PIC (include/ribbit_hip.h has the contract, kernels.h the launch).  No record is
// read and there is no floating point.
//   marker_alleles_kernel   a workgroup of four wavefronts takes ALLELE_RUN = 16 consecutive markers at a time.
//                           Load: the matrix is sample-major, so the 16 markers' cells of one sample are 64 contiguous bytes; the
//                           256 lanes read 16 samples by 16 markers per pass (lane = 16 sample + marker) and write them transposed
//                           into LDS, a row of P = alleles_keys(S) words per marker.  No lane strides by the matrix's pitch.  Row q
//                           is rotated by q words (Row below), so that the 16 markers of one sample fall into 16 banks.
//                           Per marker, one wavefront (wavefront w takes rows w, w + 4, w + 8, w + 12):
//                             kinds    the lanes walk the S cells: typed, absent, several, over, same, off_step as lane counts and
//                                      one butterfly sum each; the cell becomes its sort key in place, the size of a typed cell and
//                                      NO_KEY = 2^32 - 1 for everything else and for the padding S .. P, which so sorts behind a
//                                      size of 2^31 - 1
//                             sort     bitonic over the row's P keys, as primer_products.hip sorts its site lists; the four
//                                      wavefronts take the same barriers
//                             runs     the typed keys are the first t; a lane whose key differs from the one before it is a head
//                                      and bisects [i + 1, t) for its run's end; c = the run's length adds to Q = sum c^2, F = sum c^4
//                                      and the allele count, and (c << 32 | ~size) goes into a 64-bit maximum: the largest count,
//                                      of equals the least size.  Butterflies in 64 bits; min and max are keys 0 and t - 1.
//                           Lane 0 stores the record.  A row with designed <= 0 is sixteen zeros.
// Bounds: a cell is read at s pitch + i with s < S and i < m <= pitch; an LDS index is row q < 16 times P plus a word below P; the
// bisection stays in [i + 1, t] and reads below t <= S <= P; a record is written at i < m.  t <= 1024: t^4 <= 2^40.
#include <hip/hip_runtime.h>

#include "row_kernels.h"

namespace rb {

namespace {

constexpr int ALLELE_THREADS = 256, ALLELE_WAVES = ALLELE_THREADS / 64;
constexpr int64_t ALLELE_MAX_BLOCKS = 4096;
constexpr uint32_t NO_KEY = 0xffffffffu;
static_assert(ALLELE_RUN == 16 && ALLELE_RUN % ALLELE_WAVES == 0, "16 markers are 64 bytes of a sample's row; every wavefront takes as many");
static_assert(sizeof(RibbitRowAlleles) == 64, "twelve ints and two words of 64 bits");

// row q of the tile: word i lies at (i + q) mod P
struct Row {
    uint32_t *base;
    int rot, mask;
    __device__ uint32_t &operator[](int i) const { return base[(i + rot) & mask]; }
};

__device__ inline unsigned long long wave_total(unsigned long long v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;      // (every lane's)
}
__device__ inline unsigned long long wave_most(unsigned long long v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned long long o = __shfl_xor(v, d);
        v = o > v ? o : v;
    }
    return v;
}

__global__ __launch_bounds__(ALLELE_THREADS) void marker_alleles_kernel(const int32_t *__restrict__ cells, int64_t pitch, int S, int64_t m, const int32_t *__restrict__ designed,
                                                                         const int32_t *__restrict__ motif_lengths, int P, RibbitRowAlleles *__restrict__ out) {
    extern __shared__ uint32_t tile[];      // ALLELE_RUN rows of P words
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t runs = (m + ALLELE_RUN - 1) / ALLELE_RUN;
    for (int64_t run = blockIdx.x; run < runs; run += gridDim.x) {
        const int64_t first = run * ALLELE_RUN;
        {      // the 16 markers' cells of 16 samples per pass, transposed
            const int q = tid & (ALLELE_RUN - 1);
            const bool marker = first + q < m;
            const Row row{tile + q * P, q, P - 1};
            for (int s = tid / ALLELE_RUN; s < S; s += ALLELE_THREADS / ALLELE_RUN) row[s] = marker ? (uint32_t)cells[(int64_t)s * pitch + first + q] : 0u;
        }
        __syncthreads();
        for (int q = wave; q < ALLELE_RUN; q += ALLELE_WAVES) {      // (four turns for every wavefront)
            const int64_t i = first + q;
            const bool marker = i < m;
            const int32_t des = marker ? designed[i] : 0;
            const bool pair = des > 0;
            const int32_t step = pair ? motif_lengths[i] : 1;      // (>= 1: the host has checked it)
            const Row row{tile + q * P, q, P - 1};
            unsigned long long typed = 0, absent = 0, several = 0, over = 0, same = 0, off = 0;
            for (int s = lane; s < P; s += 64) {
                uint32_t key = NO_KEY;
                if (s < S) {
                    const int32_t c = (int32_t)row[s];
                    if (c > 0) {
                        key = (uint32_t)c;
                        ++typed;
                        if (pair) {      // (both positive: the difference is an int)
                            same += c == des;
                            off += (c - des) % step != 0;
                        }
                    } else {
                        absent += c == 0;
                        several += c == -1;
                        over += c == -2;
                    }
                }
                row[s] = key;
            }
            __syncthreads();
            for (int k = 2; k <= P; k <<= 1)
                for (int j = k >> 1; j > 0; j >>= 1) {
                    for (int a = lane; a < P; a += 64) {
                        const int b = a ^ j;
                        if (b > a) {
                            const uint32_t x = row[a], y = row[b];
                            if ((x > y) == ((a & k) == 0)) { row[a] = y; row[b] = x; }
                        }
                    }
                    __syncthreads();
                }
            const int t = (int)wave_total(typed);
            unsigned long long Q = 0, F = 0, heads = 0, most = 0;
            for (int a = lane; a < t; a += 64) {
                const uint32_t key = row[a];
                if (a > 0 && row[a - 1] == key) continue;
                int lo = a + 1, hi = t;      // the first index behind a whose key is another, or t
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (row[mid] == key) lo = mid + 1; else hi = mid;
                }
                const unsigned long long c = (unsigned long long)(lo - a);
                Q += c * c;
                F += c * c * c * c;
                ++heads;
                const unsigned long long mine = c << 32 | (unsigned long long)(NO_KEY - key);
                most = mine > most ? mine : most;
            }
            Q = wave_total(Q);
            F = wave_total(F);
            heads = wave_total(heads);
            most = wave_most(most);
            absent = wave_total(absent);
            several = wave_total(several);
            over = wave_total(over);
            same = wave_total(same);
            off = wave_total(off);
            if (lane == 0 && marker) {
                RibbitRowAlleles r{};
                if (pair) {
                    const long long tt = (long long)t * t, q = (long long)Q;
                    r.typed = t;
                    r.absent = (int32_t)absent;
                    r.several = (int32_t)several;
                    r.over = (int32_t)over;
                    r.alleles = (int32_t)heads;
                    if (t > 0) {
                        r.min_size = (int32_t)row[0];
                        r.max_size = (int32_t)row[t - 1];
                        r.major_size = (int32_t)(NO_KEY - (uint32_t)(most & 0xffffffffull));
                        r.major_count = (int32_t)(most >> 32);
                    }
                    r.same = (int32_t)same;
                    r.off_step = (int32_t)off;
                    r.het_num = tt - q;
                    r.pic_num = tt * tt - tt * q - q * q + (long long)F;
                }
                out[i] = r;
            }
        }
        __syncthreads();      // (the rows are read to the end before the next run's cells land)
    }
}

}  // namespace

AllelesLayout alleles_layout(int64_t m) {
    AllelesLayout at{};
    WorkCarver w;
    at.rows = w.take((size_t)m * sizeof(RibbitRowAlleles));
    w.close(at, 0);
    return at;
}

hipError_t launch_marker_alleles(const int32_t *cells, int64_t pitch, int64_t n_samples, int64_t m, const int32_t *designed, const int32_t *motif_lengths, uint8_t *work,
                                 size_t work_bytes, const AllelesLayout &at, hipStream_t stream) {
    if (work_bytes < at.bytes || m < 1 || pitch < m || n_samples < 1 || n_samples > RIBBIT_ALLELES_MAX_SAMPLES) return hipErrorInvalidValue;
    const int P = alleles_keys(n_samples);
    const int64_t runs = (m + ALLELE_RUN - 1) / ALLELE_RUN;
    hipLaunchKernelGGL(marker_alleles_kernel, dim3((unsigned)std::min(runs, ALLELE_MAX_BLOCKS)), dim3(ALLELE_THREADS), (size_t)ALLELE_RUN * P * sizeof(uint32_t), stream, cells,
                       pitch, (int)n_samples, m, designed, motif_lengths, P, region<RibbitRowAlleles>(work, at.rows));
    return hipGetLastError();
}

}  // namespace rb
