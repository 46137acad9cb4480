// bfhip_block.h -- the two workgroup-level reductions of the post-sampling statistics (bfhip_sit.hip, bfhip_refit.hip,
// bfhip_acor.hip, bfhip_diag.hip, bfhip_psis.hip).  Both have an order fixed by the shape alone, so a kernel's bits do not depend on
// which of them it goes through: only the shape is shared, every kernel brings its own merge.
#pragma once
#include "bfhip_common.h"

struct BfSum { __device__ double operator()(double a, double b) const { return a + b; } };
struct BfMax { __device__ double operator()(double a, double b) const { return fmax(a, b); } };   // (fmax / fmin pass over a NaN)
struct BfMin { __device__ double operator()(double a, double b) const { return fmin(a, b); } };

// Halving tree over the N threads' K-tuples v[0 .. K) in the LDS slots slot[k * N + thread]: at each of the log2 N levels thread
// t < o merges slot t + o into slot t, o = N / 2, N / 4, ..., 1; slot t is the merge's first operand.  A tuple's merge(a, b) updates
// a in place; one double's merge(a, b) takes and returns values.  The result is left in v of every thread.  Called by all N threads
// of the workgroup.
// UPPER_FIRST (one double): slot t + o is read before slot t.  The number is the same; but the hardware's add keeps the first
// operand's NaN of two, and the compiler puts the value read first there whatever the source says.  A tree that was written
// `red[t] += red[t + o]` (the right side is evaluated first) therefore keeps the upper slot's NaN, one written `a + b` on two named
// reads the lower slot's, and each kernel says here which of the two it has always been.  Nothing but the compiler's habit holds
// this: after a change of toolchain rerun tools/stats_digest.py against the library of the old one (its inputs hold both NaNs).
template <int N, int K, bool UPPER_FIRST = false, typename Merge>
__device__ inline void bf_block_tree(double *v, double *slot, Merge merge) {
    static_assert((N & (N - 1)) == 0, "a halving tree");
    const int t = threadIdx.x;
    __syncthreads();   // (the slots may still be read from the previous reduction)
#pragma unroll
    for (int k = 0; k < K; ++k) slot[k * N + t] = v[k];
    __syncthreads();
    for (int o = N / 2; o > 0; o >>= 1) {
        if constexpr (K == 1) {
            if (t < o) {
                if constexpr (UPPER_FIRST) {
                    const double hi = slot[t + o], lo = slot[t];
                    slot[t] = merge(lo, hi);
                } else {
                    const double lo = slot[t], hi = slot[t + o];
                    slot[t] = merge(lo, hi);
                }
            }
        } else if (t < o) {
            double a[K], b[K];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                a[k] = slot[k * N + t];
                b[k] = slot[k * N + t + o];
            }
            merge(a, b);
#pragma unroll
            for (int k = 0; k < K; ++k) slot[k * N + t] = a[k];
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = slot[k * N];
}

// the tree of one double per thread: op(a, b) -> the merged value
template <int N, bool UPPER_FIRST = false, typename Op>
__device__ inline double bf_block_reduce(double v, double *slot, Op op) {
    bf_block_tree<N, 1, UPPER_FIRST>(&v, slot, op);
    return v;
}

// Ordered fold of a column's row slices: a workgroup of 256 threads is BF_SLICES slices x 16 columns and red[i * 16 + b] holds
// slice i's value of column b (stored, and a barrier passed, by the caller).  Returns op(... op(op(start, red[i0]), red[i0 + 1]) ...,
// red[15]), i ascending, the running value always op's first operand (which of two NaNs a sum keeps depends on it).  Slice 0
// folding the others onto its own value passes (its value, 1); a fold from a literal is (0., 0): the two differ for a column of -0.
#define BF_SLICES 16
template <typename Op>
__device__ inline double bf_slice_fold(double start, int i0, const double *red, int b, Op op) {
    for (int i = i0; i < BF_SLICES; ++i) start = op(start, red[i * 16 + b]);
    return start;
}
