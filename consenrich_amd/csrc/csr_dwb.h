// csr_dwb.h -- the stationary-null dependent wild bootstrap (DWB) panel behind the ROCCO budgets, bit for bit what the
// reference computes (pyx:9283-9424 `cGenerateDWBMultipliersFromNoise`, `cApplyStationaryNullDWB`, `cStationaryNullDWBDraw`;
// peaks.py:593-762 the two bootstrap loops of `_calibrateStationaryNullDWB`).
//
// A draw is u[i] = sum_j noise[i + j] w[j] (2 maxLag + 1 taps), standardised by its own mean and sd, multiplied into a template
// and re-centred.  The natives accumulate every sum in index order and float64 addition is not associative, so:
//   k_dwb_movsum  the stencil, parallel over (chain, draw, i): the taps of one output in ascending j with a separate multiply
//                 and add, from 0.0 (the library is built with -ffp-contract=off); noise tile + halo and the weights in LDS;
//   k_dwb_walk    ONE LANE per (chain, draw) walks its row three times in index order (mean; squared deviations; product with
//                 the template and its mean), DWB_WR draws of one chain per wavefront.  Rows are staged through LDS in tiles
//                 of DWB_WT values with coalesced loads (lane = element), double-buffered through registers, and read back
//                 transposed (lane = row); k_dwb_centre then subtracts each row's mean of the products;
//   k_dwb_select  the exact order statistics of a row at up to DWB_MAX_RANKS ranks: a byte-wise radix select like csr_gain.h's,
//                 on a plain double array, one workgroup per row, eight passes inside one launch;
//   k_dwb_tail    count(x > offset) and the sum of clip((x - offset) / scale, 0, inf) in NumPy's summation order: one thread per
//                 (chunk of 8192, z) evaluates NumPy's pairwise tree of that chunk (np_chunk_sum_f of csr_np_order.h over the
//                 excess-and-count element); k_dwb_tail_fold folds the chunk sums in ascending order and divides by n.
// Nothing here waits on another workgroup: every dependency is a kernel boundary, every loop bound is known at launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "csr_np_order.h"

namespace csr {

constexpr int DWB_ST = 256;             // outputs per workgroup of the stencil
constexpr int DWB_MAX_LAG = 512;        // largest maxLag (qs at bandwidth 64; bartlett / parzen up to bandwidth 512)
constexpr int DWB_WT = 256;             // values per row and LDS tile of the walk (fetched 64 at a time: lane = element)
constexpr int DWB_WR = 16;              // rows (draws) per wavefront of the walk
constexpr int DWB_MAX_RANKS = 16;       // order statistics per row
constexpr int DWB_MAX_Z = 16;           // (offset, scale) pairs per row

struct DwbChain {
    int64_t off, n;         // bins [off, off + n) of a row of the concatenated layout (off is a multiple of 64)
    int64_t stride;         // n + 2 maxLag: draw b reads noise[b * stride, (b + 1) * stride)
    int maxLag, wOff;       // weights w[wOff .. wOff + 2 maxLag]
};

// rows[g * rowLen + chain.off + i]: the moving sums of draw d0 + g
__global__ __launch_bounds__(DWB_ST) void k_dwb_movsum(const DwbChain *__restrict__ chains, const double *__restrict__ noise,
                                                       const double *__restrict__ wts, double *__restrict__ rows, int64_t rowLen,
                                                       int64_t d0) {
    __shared__ double sN[DWB_ST + 2 * DWB_MAX_LAG];
    __shared__ double sW[2 * DWB_MAX_LAG + 1];
    const DwbChain ch = chains[blockIdx.z];
    const int64_t i0 = (int64_t)blockIdx.x * DWB_ST;
    if (i0 >= ch.n) return;             // (uniform per workgroup: the grid is sized for the longest chain)
    const int t = threadIdx.x, taps = 2 * ch.maxLag + 1;
    const double *z = noise + (d0 + blockIdx.y) * ch.stride;
    const int64_t have = ch.stride - i0;            // values of this draw's slice from i0 on
    const int need = DWB_ST + 2 * ch.maxLag;
    for (int k = t; k < need; k += DWB_ST) sN[k] = k < have ? z[i0 + k] : 0.0;
    for (int k = t; k < taps; k += DWB_ST) sW[k] = wts[ch.wOff + k];
    __syncthreads();
    if (i0 + t >= ch.n) return;
    double v = 0.0;
    for (int j = 0; j < taps; ++j) {
        const double prod = sN[t + j] * sW[j];
        v = v + prod;
    }
    rows[(int64_t)blockIdx.y * rowLen + ch.off + i0 + t] = v;
}

// One wavefront: rows g0 .. g0 + nl - 1 (nl <= DWB_WR) of one chain, lane r walking row r.  standardise: the rows hold moving sums
// and become multipliers (pyx:9365-9379); apply: multiply into the template (pyx:9405-9407); the mean of the products goes to
// means[chain * nRows + row] and k_dwb_centre subtracts it (pyx:9408-9411).  A tile of DWB_WT values per row is fetched into
// registers (coalesced: lane = element) while the previous tile is walked, then stored to LDS and read back transposed.
struct DwbWalkArgs {
    const DwbChain *chains;
    const double *tmpl;     // concatenated layout (apply)
    double *rows;
    double *means;
    int64_t rowLen;
    int nRows;              // rows in the buffer
    int standardise, apply;
};
__global__ __launch_bounds__(64) void k_dwb_walk(DwbWalkArgs a) {
    constexpr int K = DWB_WT / 64;
    __shared__ double sT[DWB_WR][DWB_WT + 1];
    __shared__ double sTm[DWB_WT];
    const DwbChain ch = a.chains[blockIdx.y];
    const int lane = threadIdx.x, g0 = blockIdx.x * DWB_WR;
    const int nl = a.nRows - g0 < DWB_WR ? a.nRows - g0 : DWB_WR;
    const int64_t n = ch.n;
    double *base = a.rows + (int64_t)g0 * a.rowLen + ch.off;
    const double *tm = a.tmpl + ch.off;
    const bool live = lane < nl;
    double reg[DWB_WR * K], regT[K];
    auto fetch = [&](int64_t t0, bool withTmpl) {
#pragma unroll
        for (int r = 0; r < DWB_WR; ++r)
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int64_t i = t0 + k * 64 + lane;
                reg[r * K + k] = (r < nl && i < n) ? base[(int64_t)r * a.rowLen + i] : 0.0;
            }
        if (withTmpl)
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int64_t i = t0 + k * 64 + lane;
                regT[k] = i < n ? tm[i] : 0.0;
            }
    };
    auto stash = [&](bool withTmpl) {
#pragma unroll
        for (int r = 0; r < DWB_WR; ++r)
#pragma unroll
            for (int k = 0; k < K; ++k) sT[r][k * 64 + lane] = reg[r * K + k];
        if (withTmpl)
#pragma unroll
            for (int k = 0; k < K; ++k) sTm[k * 64 + lane] = regT[k];
    };
    const int row = live ? lane : 0;
    // the steps of one tile; a full tile is unrolled so that the LDS reads run ahead of the dependent adds
    auto steps = [&](int cnt, auto body) {
        if (cnt == DWB_WT) {
#pragma unroll 32
            for (int j = 0; j < DWB_WT; ++j) body(j);
        } else
            for (int j = 0; j < cnt; ++j) body(j);
    };
    double mean = 0.0, sd = 0.0;
    bool flat = false;
    if (a.standardise) {
        double acc = 0.0;
        fetch(0, false);
        for (int64_t t0 = 0; t0 < n; t0 += DWB_WT) {
            const int cnt = (int)(n - t0 < DWB_WT ? n - t0 : DWB_WT);
            stash(false);
            __syncthreads();
            if (t0 + DWB_WT < n) fetch(t0 + DWB_WT, false);     // in flight while this tile is walked
            steps(cnt, [&](int j) { acc = acc + sT[row][j]; });
            __syncthreads();
        }
        mean = __ddiv_rn(acc, (double)n);
        if (n >= 2) {
            double var = 0.0;
            fetch(0, false);
            for (int64_t t0 = 0; t0 < n; t0 += DWB_WT) {
                const int cnt = (int)(n - t0 < DWB_WT ? n - t0 : DWB_WT);
                stash(false);
                __syncthreads();
                if (t0 + DWB_WT < n) fetch(t0 + DWB_WT, false);
                steps(cnt, [&](int j) {
                    const double d = sT[row][j] - mean;
                    const double sq = d * d;
                    var = var + sq;
                });
                __syncthreads();
            }
            sd = __dsqrt_rn(__ddiv_rn(var, (double)(n - 1)));
        }
        flat = !isfinite(sd) || sd <= 2.2250738585072014e-308;
    }
    double acc2 = 0.0;
    const bool ap = a.apply != 0;
    fetch(0, ap);
    for (int64_t t0 = 0; t0 < n; t0 += DWB_WT) {
        const int cnt = (int)(n - t0 < DWB_WT ? n - t0 : DWB_WT);
        stash(ap);
        __syncthreads();
        if (t0 + DWB_WT < n) fetch(t0 + DWB_WT, ap);
        if (live)
            steps(cnt, [&](int j) {
                double m = sT[row][j];
                if (a.standardise) m = flat ? 1.0 : __ddiv_rn(m - mean, sd);
                if (ap) {
                    m = sTm[j] * m;
                    acc2 = acc2 + m;
                }
                sT[row][j] = m;
            });
        __syncthreads();
        for (int r = 0; r < nl; ++r)
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int64_t i = t0 + k * 64 + lane;
                if (i < n) base[(int64_t)r * a.rowLen + i] = sT[r][k * 64 + lane];
            }
        __syncthreads();
    }
    if (ap && live) a.means[(int64_t)blockIdx.y * a.nRows + g0 + lane] = __ddiv_rn(acc2, (double)n);
}
// grid (ceil(longest / 256), rows, chains): row[i] -= mean of the row's products
__global__ __launch_bounds__(256) void k_dwb_centre(const DwbChain *__restrict__ chains, double *__restrict__ rows,
                                                    const double *__restrict__ means, int64_t rowLen, int nRows) {
    const DwbChain ch = chains[blockIdx.z];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= ch.n) return;
    double *p = rows + (int64_t)blockIdx.y * rowLen + ch.off + i;
    *p = *p - means[(int64_t)blockIdx.z * nRows + blockIdx.y];
}

// ---- exact order statistics of every row (on np_key: -0.0 sorts before +0.0) --------------------------------------------------
// grid (rows, chains); ranks[chain][nRanks] (-1 = unused, answered with NaN); out[(chain * outRows + d0 + row) * nRanks + q]
__global__ __launch_bounds__(256) void k_dwb_select(const DwbChain *__restrict__ chains, const double *__restrict__ rows,
                                                    int64_t rowLen, const long long *__restrict__ ranks, int nRanks,
                                                    double *__restrict__ out, int64_t outRows, int64_t d0) {
    __shared__ unsigned int h[DWB_MAX_RANKS][256];
    __shared__ int grp[DWB_MAX_RANKS];
    __shared__ unsigned long long pre[DWB_MAX_RANKS];
    __shared__ long long rk[DWB_MAX_RANKS];
    const DwbChain ch = chains[blockIdx.y];
    const double *x = rows + (int64_t)blockIdx.x * rowLen + ch.off;
    const int t = threadIdx.x;
    if (t < DWB_MAX_RANKS) {
        long long r = t < nRanks ? ranks[blockIdx.y * nRanks + t] : -1;
        if (r >= ch.n) r = -1;
        rk[t] = r;
        pre[t] = 0ull;
    }
    __syncthreads();
    for (int pass = 0; pass < 8; ++pass) {
        for (int i = t; i < DWB_MAX_RANKS * 256; i += 256) (&h[0][0])[i] = 0u;
        if (t == 0) radix_groups(rk, pre, DWB_MAX_RANKS, grp);
        __syncthreads();
        const int shift = 56 - 8 * pass;
        for (int64_t k = t; k < ch.n; k += 256) {
            const unsigned long long key = np_key(x[k]);
            const unsigned long long hi = pass == 0 ? 0ull : key >> (shift + 8);
            const unsigned int digit = (unsigned int)(key >> shift) & 255u;
            for (int q = 0; q < nRanks; ++q)
                if (grp[q] == q && hi == pre[q]) atomicAdd(&h[q][digit], 1u);
        }
        __syncthreads();
        long long newRank = -1;
        unsigned long long newPre = 0ull;
        if (t < DWB_MAX_RANKS && grp[t] >= 0) {
            long long before;
            const int digit = radix_pick_digit(h[grp[t]], rk[t], &before);
            newPre = (pre[t] << 8) | (unsigned long long)digit;
            newRank = rk[t] - before;
        }
        __syncthreads();
        if (t < DWB_MAX_RANKS && grp[t] >= 0) {
            pre[t] = newPre;
            rk[t] = newRank;
        }
        __syncthreads();
    }
    if (t < nRanks)
        out[((int64_t)blockIdx.y * outRows + d0 + blockIdx.x) * nRanks + t] =
            grp[t] >= 0 ? np_unkey(pre[t]) : __longlong_as_double(0x7ff8000000000000ll);
}

// ---- tail statistics -------------------------------------------------------------------------------------------------------
// the element of the tail statistics: counts x > off on the way
struct DwbExcess {
    double off, s;
    long long &cnt;
    __device__ __forceinline__ double operator()(double x) {
        cnt += x > off;
        return np_excess(x, off, s);
    }
};
struct DwbTailArgs {
    const DwbChain *chains;
    const double *rows;
    int64_t rowLen;
    const double *off, *scale;  // [chain][nZ] (scale already max(scale, DBL_MIN))
    int nZ;
    int64_t maxChunks;          // chunks of the longest chain
    double *partSum;            // [chain][row][maxChunks][nZ]
    long long *partCnt;
    int nRows;
    long long *cnt;             // [(chain * outRows + d0 + row) * nZ + z]
    double *soft;
    int64_t outRows, d0;
};
// grid (ceil(maxChunks * nZ / 64), rows, chains); one thread per (chunk, z)
__global__ __launch_bounds__(64) void k_dwb_tail(DwbTailArgs a) {
    const DwbChain ch = a.chains[blockIdx.z];
    const int64_t pair = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const int64_t chunk = pair / a.nZ;
    const int z = (int)(pair % a.nZ);
    const int64_t nChunks = (ch.n + NP_CHUNK - 1) / NP_CHUNK;
    if (chunk >= nChunks) return;
    const double *x = a.rows + (int64_t)blockIdx.y * a.rowLen + ch.off + chunk * NP_CHUNK;
    const int64_t left = ch.n - chunk * NP_CHUNK;
    const int len = (int)(left < NP_CHUNK ? left : NP_CHUNK);
    long long cnt = 0;
    DwbExcess f{a.off[blockIdx.z * a.nZ + z], a.scale[blockIdx.z * a.nZ + z], cnt};
    const double s = np_chunk_sum_f(x, len, f);
    const int64_t slot = ((((int64_t)blockIdx.z * a.nRows + blockIdx.y) * a.maxChunks) + chunk) * a.nZ + z;
    a.partSum[slot] = s;
    a.partCnt[slot] = cnt;
}
// one thread per (chain, row, z): the chunk sums in ascending order, then / n
__global__ __launch_bounds__(64) void k_dwb_tail_fold(DwbTailArgs a, int nChains) {
    const int64_t id = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const int64_t total = (int64_t)nChains * a.nRows * a.nZ;
    if (id >= total) return;
    const int z = (int)(id % a.nZ);
    const int row = (int)((id / a.nZ) % a.nRows);
    const int c = (int)(id / ((int64_t)a.nZ * a.nRows));
    const DwbChain ch = a.chains[c];
    const int64_t nChunks = (ch.n + NP_CHUNK - 1) / NP_CHUNK;
    const int64_t slot0 = (((int64_t)c * a.nRows + row) * a.maxChunks) * a.nZ + z;
    double s = a.partSum[slot0];
    long long cnt = a.partCnt[slot0];
    for (int64_t k = 1; k < nChunks; ++k) {
        s = s + a.partSum[slot0 + k * a.nZ];
        cnt += a.partCnt[slot0 + k * a.nZ];
    }
    const int64_t o = ((int64_t)c * a.outRows + a.d0 + row) * a.nZ + z;
    a.soft[o] = __ddiv_rn(s, (double)ch.n);
    a.cnt[o] = cnt;
}

}  // namespace csr
