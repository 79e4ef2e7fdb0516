// repeats.hip -- every row's bases with their flanks as FASTA entries (api_repeats.cpp: ribbit_hip_repeat_sequences).  On the
// handle's stream:
//   offsets: the entry length of every row (inside the scan's input iterator) -> exclusive offsets, int64 (rocPRIM scan)
//   pick:    one lane: k, the rows whose text fits the budget, and their byte count (the only values the host waits for)
//   spans:   one lane per REPEAT_SPAN bytes of output: the row that holds the span's first byte (binary search of the offsets)
//   format:  one workgroup per span: the span's rows' headers into LDS (one lane per row), then 16 output bytes per lane,
//            stored as one dwordx4; the body bytes come from two aligned 16-byte loads and a 128-bit funnel shift
// Entry of row i, in 64-bit arithmetic (include/ribbit_hip.h):
//   ">" name ":" s' "-" e' " flank=" (s' - lo) "," (hi - e') "\n" bases[lo, hi) "\n"
// s' and e' are at most max(s, e) <= INT32_MAX and the flank lengths at most F <= INT32_MAX: every number has 1 to 10 digits.
#include <cstring>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "kernels.h"

namespace rb {

namespace {

constexpr int REP_THREADS = 256;
static_assert(REPEAT_SPAN == 16 * REP_THREADS, "a format workgroup writes one span, 16 bytes per lane");
// An entry is at least 17 bytes (">:0-0 flank=0,0\n\n"), so the rows that meet one span are at most those that lie inside it
// plus the two at its ends.
constexpr int REP_MIN_ENTRY = 17;
constexpr int REP_MAX_ROWS = (int)(REPEAT_SPAN / REP_MIN_ENTRY) + 2;
static_assert(REP_MAX_ROWS <= REP_THREADS, "one lane per row of a span");
// the header after the name: ":" s' "-" e' " flank=" left "," right "\n", at most 4 * 10 + 11 bytes
constexpr int REP_TAIL = 52;

__host__ __device__ inline int64_t imin(int64_t a, int64_t b) { return a < b ? a : b; }
__host__ __device__ inline int64_t imax(int64_t a, int64_t b) { return a < b ? b : a; }

__host__ __device__ inline int digits(uint32_t v) {
    int d = 1;
    for (uint32_t p = 10; d < 10 && v >= p; p *= 10) ++d;
    return d;
}

// the clipped bounds of a row and the parts of its entry's length
struct RowBounds {
    int64_t s, e, lo, hi;
    int32_t head;        // header bytes, name and '\n' included
    __host__ __device__ RowBounds(int32_t s_in, int32_t e_in, int64_t length, int32_t flank, int32_t name_len) {
        s = imin(imax(s_in, 0), length);
        e = imin(imax(e_in, s), length);
        lo = imax(s - flank, 0);
        hi = imin(e + flank, length);
        head = 12 + name_len + digits((uint32_t)s) + digits((uint32_t)e) + digits((uint32_t)(s - lo)) + digits((uint32_t)(hi - e));
    }
    __host__ __device__ int64_t entry() const { return head + (hi - lo) + 1; }
};

struct EntryLength {
    const int32_t *iv;
    int64_t length;
    int32_t flank, name_len;
    __host__ __device__ int64_t operator()(int64_t i) const { return RowBounds(iv[2 * i], iv[2 * i + 1], length, flank, name_len).entry(); }
};

__global__ void repeat_pick_kernel(const int64_t *__restrict__ off, int64_t m, int64_t budget, int64_t *__restrict__ pick) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int64_t lo = 0, hi = m + 1;      // off[lo] <= budget (off[0] = 0), off[hi] > budget or hi = m + 1
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (off[mid] <= budget) lo = mid; else hi = mid;
    }
    const int64_t k = max(lo, (int64_t)1);
    pick[0] = k;
    pick[1] = off[k];
}

// span_row[b] = the row whose entry holds byte b * REPEAT_SPAN (the last byte for b = spans)
__global__ void __launch_bounds__(REP_THREADS) repeat_span_kernel(const int64_t *__restrict__ off, int64_t k, int64_t total, int64_t spans,
                                                                  int32_t *__restrict__ span_row) {
    const int64_t b = (int64_t)blockIdx.x * REP_THREADS + threadIdx.x;
    if (b > spans) return;
    const int64_t o = min(b * REPEAT_SPAN, total - 1);
    int64_t lo = 0, hi = k;          // off[lo] <= o < off[hi]
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (off[mid] <= o) lo = mid; else hi = mid;
    }
    span_row[b] = (int32_t)lo;
}

__device__ inline int put_number(uint8_t *t, int at, uint32_t v) {
    const int d = digits(v);
    for (int i = d - 1; i >= 0; --i) {
        t[at + i] = (uint8_t)('0' + v % 10);
        v /= 10;
    }
    return at + d;
}

__device__ inline int put_text(uint8_t *t, int at, const char *s) {
    for (; *s; ++s) t[at++] = (uint8_t)*s;
    return at;
}

// Workgroup b writes output bytes [b * SPAN, (b + 1) * SPAN) of the batch.  Its rows are span_row[b] .. span_row[b + 1]; lane t
// builds row span_row[b] + t's entry offset, the record index its body starts from, its header length and the header after the
// name into LDS.  Then lane t writes bytes [c, c + 16), c = b * SPAN + 16 t: it finds row j with off[j] <= c < off[j + 1] in LDS.
// An entry is longer than 16 bytes, so the 16 bytes meet row j and at most row j + 1; row j + 1's header is at least 16 bytes, so
// only row j can contribute body bytes, and those are bases[c + base_j .. c + base_j + 16) for the one base_j = lo_j - off_j -
// head_j.  They come from two aligned 16-byte loads and one 128-bit funnel shift when both loads lie in the record, else from
// byte loads of the indices in [0, length).  Every other byte is '>', a name byte (global, small), a header byte from LDS or '\n'.
__global__ void __launch_bounds__(REP_THREADS) repeat_format_kernel(const uint8_t *__restrict__ ascii, int64_t length,
                                                                    const int32_t *__restrict__ iv, const int64_t *__restrict__ off,
                                                                    int64_t total, int32_t flank, const char *__restrict__ name,
                                                                    int32_t name_len, const int32_t *__restrict__ span_row,
                                                                    uint4 *__restrict__ out) {
    __shared__ int64_t s_off[REP_MAX_ROWS + 1];
    __shared__ int64_t s_base[REP_MAX_ROWS];
    __shared__ int32_t s_head[REP_MAX_ROWS];
    __shared__ uint8_t s_tail[REP_MAX_ROWS][REP_TAIL];
    const int64_t spans = (total + REPEAT_SPAN - 1) / REPEAT_SPAN;
    const int t = threadIdx.x;
    for (int64_t b = blockIdx.x; b < spans; b += gridDim.x) {
        const int32_t r0 = span_row[b];
        const int nrows = min(span_row[b + 1] - r0 + 1, REP_MAX_ROWS);      // (never clipped: see REP_MAX_ROWS)
        if (t < nrows) {
            const int64_t r = r0 + t;
            const RowBounds rb(iv[2 * r], iv[2 * r + 1], length, flank, name_len);
            s_off[t] = off[r];
            if (t == nrows - 1) s_off[t + 1] = off[r + 1];
            s_base[t] = rb.lo - off[r] - rb.head;
            s_head[t] = rb.head;
            uint8_t *tail = s_tail[t];
            int at = 0;
            tail[at++] = ':';
            at = put_number(tail, at, (uint32_t)rb.s);
            tail[at++] = '-';
            at = put_number(tail, at, (uint32_t)rb.e);
            at = put_text(tail, at, " flank=");
            at = put_number(tail, at, (uint32_t)(rb.s - rb.lo));
            tail[at++] = ',';
            at = put_number(tail, at, (uint32_t)(rb.hi - rb.e));
            tail[at] = '\n';
        }
        __syncthreads();
        const int64_t c = b * REPEAT_SPAN + 16 * t;
        if (c < total) {
            int lo = 0, hi = nrows;      // s_off[lo] <= c < s_off[hi]
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (s_off[mid] <= c) lo = mid; else hi = mid;
            }
            const int j = lo;
            const int64_t off_j = s_off[j], end_j = s_off[j + 1];
            const int64_t body_from = off_j + s_head[j], body_to = end_j - 1;      // output bytes of row j's body
            uint64_t r0w = 0, r1w = 0;         // bases c + base_j .. + 16, byte 0 first; outside the record: 0
            if (body_from < c + 16 && body_to > c) {
                const int64_t i0 = s_base[j] + c;
                const uintptr_t start = (uintptr_t)ascii, at = start + (uintptr_t)i0, aligned = at & ~(uintptr_t)15;
                if (i0 >= 0 && aligned >= start && aligned + 32 <= start + (uintptr_t)length) {
                    const uint4 a = *(const uint4 *)aligned, bq = *(const uint4 *)(aligned + 16);
                    uint64_t q0 = (uint64_t)a.y << 32 | a.x, q1 = (uint64_t)a.w << 32 | a.z;
                    uint64_t q2 = (uint64_t)bq.y << 32 | bq.x, q3 = (uint64_t)bq.w << 32 | bq.z;
                    const int sh_bytes = (int)(at - aligned);
                    if (sh_bytes >= 8) { q0 = q1; q1 = q2; q2 = q3; }
                    const int sh = (sh_bytes & 7) * 8;
                    r0w = sh ? (q0 >> sh) | (q1 << (64 - sh)) : q0;
                    r1w = sh ? (q1 >> sh) | (q2 << (64 - sh)) : q1;
                } else {
#pragma unroll
                    for (int k = 0; k < 16; ++k) {
                        const int64_t i = i0 + k;
                        const uint64_t v = i >= 0 && i < length ? (uint64_t)ascii[i] : 0;
                        if (k < 8) r0w |= v << (8 * k); else r1w |= v << (8 * (k - 8));
                    }
                }
            }
            uint64_t lo_w = 0, hi_w = 0;
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int64_t o = c + k;
                uint32_t v = 0;
                if (o < total) {
                    const bool next = o >= end_j;
                    const int row = next ? j + 1 : j;
                    const int64_t q = o - (next ? end_j : off_j);      // byte of the row's entry
                    if (!next && o >= body_from) {
                        v = o < body_to ? (uint32_t)((k < 8 ? r0w >> (8 * k) : r1w >> (8 * (k - 8))) & 0xff) : (uint32_t)'\n';
                    } else if (q == 0) {
                        v = '>';
                    } else if (q <= name_len) {
                        v = (uint8_t)name[q - 1];
                    } else {
                        v = s_tail[row][q - 1 - name_len];
                    }
                }
                if (k < 8) lo_w |= (uint64_t)v << (8 * k); else hi_w |= (uint64_t)v << (8 * (k - 8));
            }
            out[c >> 4] = make_uint4((uint32_t)lo_w, (uint32_t)(lo_w >> 32), (uint32_t)hi_w, (uint32_t)(hi_w >> 32));
        }
        __syncthreads();
    }
}

template <typename It>
hipError_t scan_offsets(void *scratch, size_t &bytes, It in, int64_t *off, int64_t m, hipStream_t stream) {
    return rocprim::inclusive_scan(scratch, bytes, in, off, (size_t)m, rocprim::plus<int64_t>(), stream);
}

auto entry_lengths(const int32_t *iv, int64_t length, int32_t flank, int32_t name_len) {
    return rocprim::make_transform_iterator(rocprim::make_counting_iterator<int64_t>(0), EntryLength{iv, length, flank, name_len});
}

}  // namespace

size_t repeat_scan_scratch_bytes(int64_t m) {
    size_t bytes = 0;
    (void)scan_offsets(nullptr, bytes, entry_lengths(nullptr, 0, 0, 0), (int64_t *)nullptr, m, 0);
    return bytes + 256;
}

hipError_t launch_repeat_offsets(const int32_t *iv, int64_t m, int64_t length, int32_t flank, int32_t name_len, int64_t budget,
                                 int64_t *off, int64_t *pick, void *scratch, size_t scratch_bytes, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(off, 0, sizeof(int64_t), stream);
    if (e != hipSuccess) return e;
    if ((e = scan_offsets(scratch, scratch_bytes, entry_lengths(iv, length, flank, name_len), off + 1, m, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(repeat_pick_kernel, dim3(1), dim3(64), 0, stream, off, m, budget, pick);
    return hipGetLastError();
}

void launch_repeat_format(const uint8_t *ascii, int64_t length, const int32_t *iv, const int64_t *off, int64_t k, int64_t total,
                          int32_t flank, const char *name, int32_t name_len, int32_t *span_row, uint8_t *out, hipStream_t stream) {
    if (total <= 0) return;
    const int64_t spans = (total + REPEAT_SPAN - 1) / REPEAT_SPAN;
    // (one lane per span and one more, none of them striding: no cap; one workgroup per span, striding from 256 * 64 spans on)
    hipLaunchKernelGGL(repeat_span_kernel, dim3(grid_for(spans + 1, REP_THREADS, INT32_MAX)), dim3(REP_THREADS), 0, stream, off, k, total, spans, span_row);
    hipLaunchKernelGGL(repeat_format_kernel, dim3(grid_for(spans, 1, 256 * 64)), dim3(REP_THREADS), 0, stream, ascii, length, iv, off, total, flank,
                       name, name_len, span_row, (uint4 *)out);
}

}  // namespace rb
