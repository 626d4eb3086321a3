// csr_np_order.h -- what "NumPy order" means in this library, once: the small routines every post-fit stage is gated on bit for
// bit (DESIGN section "What NumPy order means here").
//   sums     np.sum of a contiguous float64 array is the ascending fold of the pairwise sums of chunks of NP_CHUNK values; a
//            chunk's pairwise tree splits a block above 128 values at n/2 - (n/2) % 8 and sums a leaf through eight accumulators;
//   keys     the order-preserving unsigned key of a double or a float, and back;
//   values   finite, the clipped excess, np.maximum's NaN rule, NumPy's `_lerp`;
//   scans    the inclusive scan over a workgroup and the ballot rank of a flag;
//   select   the two serial steps of a byte-wise radix select;
//   kernels  one thread per chunk evaluates the chunk's tree, one thread per job folds the chunk sums.
// Whatever the code allows is __host__ __device__: tests/native/np_order_host_check.hip runs it on the CPU.  The library is built
// with -ffp-contract=off: every operation below rounds on its own.
#pragma once
#include <hip/hip_runtime.h>

namespace csr {

#define CSR_HD __host__ __device__ __forceinline__

// ---- sums ---------------------------------------------------------------------------------------------------------------------
constexpr int NP_CHUNK = 8192;          // NumPy's reduction buffer: np.sum is the ascending fold of pairwise sums of such chunks
// A block of more than 128 values splits into n2 = n/2 - (n/2) % 8 and n - n2 <= n/2 + 7.5 values, so a block at depth k of a
// chunk's tree holds fewer than NP_CHUNK / 2^k + 15: nothing splits at depth NP_STACK - 1, and the walk holds one block per depth
constexpr int NP_STACK = 8;
static_assert(NP_CHUNK / (1 << (NP_STACK - 1)) + 15 <= 128, "NP_STACK must hold the depth of one chunk's tree");

// NumPy's pairwise sum of f(x[i]) over a block of 8 <= n <= 128 values (eight strided accumulators, then the remainder in order)
// or of n < 8 values (in order, from 0.0: np.sum of a few -0.0 is +0.0); f is evaluated once per element, in the order NumPy adds.
// (Eight or more values that are ALL -0.0 sum to -0.0 here and to +0.0 in np.sum: a zero's sign, as in every stage so far)
template <class F>
CSR_HD double np_leaf_f(const double *x, int n, F &f) {
    if (n < 8) {
        double res = 0.0;
        for (int i = 0; i < n; ++i) res = res + f(x[i]);
        return res;
    }
    double r[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) r[k] = f(x[k]);
    int i = 8;
    for (; i < n - (n % 8); i += 8) {
#pragma unroll
        for (int k = 0; k < 8; ++k) r[k] = r[k] + f(x[i + k]);
    }
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res = res + f(x[i]);
    return res;
}
// The pairwise tree over n <= NP_CHUNK values: leaf(lo, len) is the sum of the block [lo, lo + len), len <= 128; the leaves are
// asked for from left to right, and a split block is its left part plus its right part.  The walk's stack -- per depth the block's
// length and, of a right part, its left sibling's sum: NP_STACK entries each -- lives where the caller puts it (registers, LDS)
template <class Leaf>
CSR_HD double np_tree(int n, Leaf &&leaf, int *len, double *left) {
    int sp = 0, pos = 0;
    unsigned right = 0u;        // bit d: the block at depth d is a right part
    len[0] = n;
    for (;;) {
        while (len[sp] > 128) {         // down to the leftmost leaf
            int n2 = len[sp] / 2;
            n2 -= n2 % 8;
            len[++sp] = n2;
            right &= ~(1u << sp);
        }
        double ret = leaf(pos, len[sp]);
        pos += len[sp];
        while (sp > 0 && ((right >> sp) & 1u)) ret = left[sp--] + ret;      // a right part closes its parent
        if (sp == 0) return ret;
        left[sp] = ret;                 // a left part: on to its sibling
        len[sp] = len[sp - 1] - len[sp];
        right |= 1u << sp;
    }
}
template <class F>
CSR_HD double np_chunk_sum_f(const double *x, int n, F &f) {
    int len[NP_STACK];
    double left[NP_STACK];
    return np_tree(n, [&](int lo, int m) { return np_leaf_f(x + lo, m, f); }, len, left);
}
// np.sum of f(x[0 .. n)), any n
template <class F>
CSR_HD double np_sum_f(const double *x, int64_t n, F f) {
    double total = 0.0;
    for (int64_t c0 = 0; c0 < n; c0 += NP_CHUNK) {
        const double part = np_chunk_sum_f(x + c0, (int)(n - c0 < NP_CHUNK ? n - c0 : NP_CHUNK), f);
        total = c0 == 0 ? part : total + part;
    }
    return total;
}
struct NpIdentity {
    CSR_HD double operator()(double x) const { return x; }
};

// ---- keys -----------------------------------------------------------------------------------------------------------------------
// Ascending order of doubles (floats) as unsigned keys, and back: monotone over everything but NaN.  -0.0 sorts before +0.0 here
// and equal to it in NumPy: a caller for whom both zeros are one value keys x + 0.0
CSR_HD unsigned long long np_key(double g) {
    const unsigned long long b = __builtin_bit_cast(unsigned long long, g);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
CSR_HD double np_unkey(unsigned long long k) {
    return __builtin_bit_cast(double, (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k);
}
CSR_HD uint32_t np_key(float v) {
    const uint32_t u = __builtin_bit_cast(uint32_t, v);
    return (u >> 31) ? ~u : (u | 0x80000000u);
}
CSR_HD float np_unkey(uint32_t k) { return __builtin_bit_cast(float, (k >> 31) ? (k & 0x7fffffffu) : ~k); }

// ---- values ---------------------------------------------------------------------------------------------------------------------
CSR_HD bool np_finite(float v) { return __builtin_fabsf(v) <= 3.402823466e+38f; }              // (false for a NaN)
CSR_HD bool np_finite(double v) { return __builtin_fabs(v) <= 1.7976931348623157e+308; }
// np.clip((x - off) / s, 0, None) of one element (np.maximum: a NaN stays, -0.0 becomes 0.0; IEEE division)
CSR_HD double np_excess(double x, double off, double s) {
    const double v = (x - off) / s;
    return (v > 0.0 || v != v) ? v : 0.0;
}
// np.maximum of two values: a NaN stays, the first one if both are
CSR_HD double np_max_nan(double a, double b) { return a != a ? a : (b != b ? b : (b > a ? b : a)); }
// numpy.lib._function_base_impl._lerp
CSR_HD double np_lerp(double a, double b, double t) {
    const double d = b - a;
    if (t >= 0.5) {
        const double s = d * (1.0 - t);
        return b - s;
    }
    const double s = d * t;
    return a + s;
}

// ---- workgroup scans --------------------------------------------------------------------------------------------------------------
// Inclusive scan of one value per thread over a workgroup of WIDTH threads (the exclusive one is the result minus v); total: the
// sum over the workgroup.  sW: WIDTH / 64 values of LDS.  Two barriers
template <int WIDTH, class T>
__device__ __forceinline__ T wg_scan(T v, T *sW, T &total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
    }
    __syncthreads();            // (sW may still be read from the previous call)
    if (lane == 63) sW[wv] = v;
    __syncthreads();
    T pre = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < WIDTH / 64; ++k) {
        const T s = sW[k];
        if (k < wv) pre += s;
        total += s;
    }
    return pre + v;
}
// The stable compaction step of a workgroup of 256 (four wavefronts): the calling thread's rank among the set flags of the
// workgroup (where its value goes, from the step's base); *total: how many flags are set.  sW: 4 ints of LDS.  Two barriers
__device__ __forceinline__ int wg_rank256(bool f, int *sW, int *total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long b = __ballot(f);
    const int pre = __popcll(b & ((1ull << lane) - 1ull));
    __syncthreads();            // (sW of the previous step has been read)
    if (lane == 0) sW[wv] = __popcll(b);
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        off += k < wv ? sW[k] : 0;
        tot += sW[k];
    }
    *total = tot;
    return off + pre;
}

// ---- the serial steps of a byte-wise radix select -------------------------------------------------------------------------------------
// Targets with equal prefixes share one histogram: grp[t] = the first target with t's prefix (-1: rank[t] < 0, the target is unused)
CSR_HD void radix_groups(const long long *rank, const unsigned long long *prefix, int T, int *grp) {
    for (int t = 0; t < T; ++t) {
        grp[t] = -1;
        if (rank[t] < 0) continue;
        grp[t] = t;
        for (int u = 0; u < t; ++u)
            if (grp[u] == u && prefix[u] == prefix[t]) { grp[t] = u; break; }
    }
}
// The digit whose cumulative count passes the rank (255 if none does); *before: the count of the digits below it
CSR_HD int radix_pick_digit(const unsigned int *hist256, long long rank, long long *before) {
    long long cum = 0;
    int digit = 255;
    for (int d = 0; d < 256; ++d) {
        const long long c = (long long)hist256[d];
        if (rank < cum + c) { digit = d; break; }
        cum += c;
    }
    *before = cum;
    return digit;
}

// ---- NumPy-order sums of many arrays ------------------------------------------------------------------------------------------------
// A Job is one array: n, data(base) = its first value, elem() = the element functor.
// grid (ceil(maxChunks / 64), jobs): part[job * maxChunks + chunk] = the pairwise tree of the chunk
template <class Job>
__global__ __launch_bounds__(64) void k_np_chunk_sums(const Job *__restrict__ jobs, const double *__restrict__ base,
                                                      double *__restrict__ part, int64_t maxChunks) {
    const Job jb = jobs[blockIdx.y];
    const int64_t chunk = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (chunk * NP_CHUNK >= jb.n) return;
    const int64_t left = jb.n - chunk * NP_CHUNK;
    auto e = jb.elem();
    part[(int64_t)blockIdx.y * maxChunks + chunk] =
        np_chunk_sum_f(jb.data(base) + chunk * NP_CHUNK, (int)(left < NP_CHUNK ? left : NP_CHUNK), e);
}
// one thread per job: the chunk sums in ascending order
template <class Job>
__global__ __launch_bounds__(64) void k_np_fold(const Job *__restrict__ jobs, int nJobs, const double *__restrict__ part,
                                                int64_t maxChunks, double *__restrict__ out) {
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j >= nJobs) return;
    const int64_t nChunks = (jobs[j].n + NP_CHUNK - 1) / NP_CHUNK;
    double s = 0.0;
    if (nChunks > 0) s = part[(int64_t)j * maxChunks];
    for (int64_t k = 1; k < nChunks; ++k) s = s + part[(int64_t)j * maxChunks + k];
    out[j] = s;
}

}  // namespace csr
