// product_walk.h -- the products of one primer pair among the sorted site lists of its two oligos, by one lane: what
// pair_products_kernel (primer_products.hip) does per pair and specific_pairs_kernel (primer_specific.hip) per pair of the two
// shortlists (include/ribbit_hip.h has the contract).  For every forward site two bisections per reverse list give the sites in
// [x + k1, x + max_product - k2]; the same walk gives `own` and `shortest_other`.  A list longer than max_sites is never read.
// first_product says where the first of those products lies (amplicons.hip: pair_amplicons_kernel).
// Included by those three .hip files only.
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

// the first product of that pair, the one with the least key (f.x, v.x + v.k, forward_of, reverse_of); the caller has found
// products > 0 with pair_products, so all four lists are complete.  A forward list ascends, so its first site with any admissible
// reverse site ends its search; the least end behind a forward site is the first reverse site of either list at or behind x + k_f.
struct FirstProduct { int32_t start, end, forward_of, reverse_of, inner_start, inner_end; };
__device__ inline FirstProduct first_product(uint32_t ua, uint32_t ub, const UniqueOligo *__restrict__ uniques, const uint32_t *__restrict__ counts,
                                             const int32_t *__restrict__ lists, int max_product, int max_sites) {
    const uint32_t u[2] = {ua, ub};
    const int k[2] = {(int)uniques[u[0]].length, (int)uniques[u[1]].length};
    FirstProduct best{-1, -1, 0, 0, -1, -1};
    int64_t best_x = INT64_MAX, best_end = INT64_MAX;
    for (int f = 0; f < 2; ++f) {
        const int32_t *F = lists + (int64_t)(2 * u[f]) * max_sites;
        const uint32_t nf = counts[2 * u[f]];
        bool found = false;
        for (uint32_t j = 0; j < nf && !found; ++j) {
            const int64_t x = F[j];
            if (x > best_x) break;
            for (int v = 0; v < 2; ++v) {
                const int32_t *V = lists + (int64_t)(2 * u[v] + 1) * max_sites;
                const int n = (int)counts[2 * u[v] + 1];
                const int from = below(V, n, x + k[f]);
                if (from >= n || (int64_t)V[from] + k[v] - x > max_product) continue;
                found = true;
                const int64_t end = (int64_t)V[from] + k[v];
                // (f and v ascend in the loops, so among equal (x, end) the first one met has the least (forward_of, reverse_of))
                if (x < best_x || (x == best_x && end < best_end)) {
                    best_x = x;
                    best_end = end;
                    best = FirstProduct{(int32_t)x, (int32_t)end, f, v, (int32_t)(x + k[f]), V[from]};
                }
            }
        }
    }
    return best;
}

}  // namespace

}  // namespace rb
