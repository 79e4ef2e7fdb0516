// product_walk.h -- the products of one primer pair among the sorted site lists of its two oligos, by one lane: what
// pair_products_kernel (primer_products.hip) does per pair and specific_pairs_kernel (primer_specific.hip) per pair of the two
// shortlists (include/ribbit_hip.h has the contract).  For every forward site two bisections per reverse list give the sites in
// [x + k1, x + max_product - k2]; the same walk gives `own` and `shortest_other`.  A list longer than max_sites is never read.
// Included by those two .hip files only.
#pragma once
#include <hip/hip_runtime.h>

#include "row_kernels.h"

namespace rb {

namespace {

struct UniqueOligo {
    unsigned long long bases;
    uint32_t length, spare;
};

// the entries of the ascending list[0, n) below v
__device__ inline int below(const int32_t *__restrict__ list, int n, int64_t v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((int64_t)list[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the pair of the unique oligos ua (the left primer) and ub (the right primer as ordered), whose own product is (a forward at
// left_start, b reverse at right_start); counts: the sites of pattern 2 u + strand, lists: max_sites slots per pattern
__device__ inline RibbitRowProducts pair_products(uint32_t ua, uint32_t ub, int32_t left_start, int32_t right_start, const UniqueOligo *__restrict__ uniques,
                                                  const uint32_t *__restrict__ counts, const int32_t *__restrict__ lists, int max_product, int max_sites) {
    RibbitRowProducts r = {};
    const uint32_t u[2] = {ua, ub};
    const int k[2] = {(int)uniques[u[0]].length, (int)uniques[u[1]].length};
    // the lists: forward of a, forward of b; reverse of a, reverse of b
    const uint32_t nf[2] = {counts[2 * u[0]], counts[2 * u[1]]}, nv[2] = {counts[2 * u[0] + 1], counts[2 * u[1] + 1]};
    r.left_forward = (int32_t)nf[0];
    r.left_reverse = (int32_t)nv[0];
    r.right_forward = (int32_t)nf[1];
    r.right_reverse = (int32_t)nv[1];
    if (max(max(nf[0], nf[1]), max(nv[0], nv[1])) > (uint32_t)max_sites) {
        r.products = -1;
        return r;
    }
    int64_t shortest = INT64_MAX;
    for (int f = 0; f < 2; ++f) {
        const int32_t *F = lists + (int64_t)(2 * u[f]) * max_sites;
        for (uint32_t j = 0; j < nf[f]; ++j) {
            const int64_t x = F[j];
            for (int v = 0; v < 2; ++v) {
                const int32_t *V = lists + (int64_t)(2 * u[v] + 1) * max_sites;
                const int n = (int)nv[v];
                // the reverse sites y with x + k_f <= y and y + k_v - x <= max_product
                const int from = below(V, n, x + k[f]), to = below(V, n, x + (int64_t)max_product - k[v] + 1);
                if (to <= from) continue;
                r.products += to - from;
                int first = from;
                if (f == 0 && v == 1 && x == left_start) {
                    const int at = below(V, n, right_start);
                    if (at >= from && at < to && V[at] == right_start) {
                        r.own = 1;
                        if (at == from) ++first;
                    }
                }
                if (first < to) shortest = min(shortest, (int64_t)V[first] + k[v] - x);
            }
        }
    }
    r.shortest_other = shortest == INT64_MAX ? 0 : (int32_t)shortest;
    return r;
}

}  // namespace

}  // namespace rb
