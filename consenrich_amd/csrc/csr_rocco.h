// csr_rocco.h -- budgeted chain peak selection (ROCCO), bit for bit what the reference's natives decide
// (pyx:8603-8716 `_solvePenalizedChainROCCO_F64`, pyx:8743-8844 `_calibrateSelectionPenaltyROCCO_F64`,
// pyx:8877-8958 `csolveChromROCCOExact`, pyx:9427-9457 `cBooleanRunBounds`, peaks.py:342-393 `consenrichStateScoreTrack`).
//
// The chain recursion is a two-state dynamic programme over the bins whose value AND tie-break (equal value: the smaller
// count wins) must be the reference's.  Floating-point addition is not associative, so no re-associated (max,+) scan over
// time reproduces either; every (chain, penalty) pair is therefore ONE LANE that runs the recursion as written, in the
// reference's operation order, with float64 adds and no contraction (the library is built with -ffp-contract=off).
// Parallelism comes from the chains of a batch and from the penalties: a bisection of the penalty that would visit D
// midpoints one after the other has only 2^D - 1 midpoints it CAN visit, all computable up front with the reference's own
// expression (lower + upper) / 2.0; they are the lanes of one wavefront (D = 6: 63 lanes), which walks the chain once.
//
// k_rocco_chain: one wavefront per (chain, group of <= 64 penalties).  The wavefront stages tiles of ROCCO_TILE scores (and
// switch costs, when they are not one constant) into LDS with coalesced 8-byte loads, double-buffered through registers;
// every lane then reads the SAME LDS address per step (a broadcast: no bank conflicts).  Lanes differ only in the penalty; the
// step is selects, no branches.  A count-only pass stores nothing but each lane's final (value, count).  The backtrace
// variant (one penalty) packs the two backtrace bits of 32 steps into a 64-bit word in registers and writes it with an
// ordinary vector store; lane 0 then traces back a word per 32 steps, writes the uint8 mask eight bins per store, and runs
// the reference's sequential unpenalised objective sum forward over the mask.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "csr_np_order.h"

namespace csr {

constexpr int ROCCO_TILE = 1024;        // steps per LDS tile (a multiple of 64 and of the 32 steps of a backtrace word)
constexpr int ROCCO_MAX_DEPTH = 8;      // speculation depth D: 2^D - 1 penalties per chain and round

// one wavefront's work: chain [off, off + n) of the concatenated arrays (off is a multiple of 64) under the penalties
// pen[penOff .. penOff + nPen); lane k's result goes to res[penOff + k]
struct RoccoJob {
    int64_t off, n;
    double gamma;           // the constant switch cost (CONSTC kernels)
    int penOff, nPen;
};
struct RoccoRes {
    double val;             // penalised objective of the best path
    double objective;       // backtrace variant: the unpenalised objective of that path (pyx:8946-8950)
    int64_t count;          // selected bins
    int64_t state;          // final state
};

// one step of pyx:8659-8695; sw = take the switch candidate (greater value, or equal value and strictly smaller count)
#define CSR_ROCCO_STEP(SV, CV, J)                                                       \
    {                                                                                   \
        const double sv_ = (SV), cv_ = (CV);                                            \
        const double sw0_ = v1 - cv_;                                                   \
        const bool t0_ = (sw0_ > v0) | ((sw0_ == v0) & (c1 < c0));                      \
        const double st1_ = (v1 + sv_) - p;                                             \
        const double sw1_ = ((v0 - cv_) + sv_) - p;                                     \
        const bool t1_ = (sw1_ > st1_) | ((sw1_ == st1_) & (c0 < c1));                  \
        const int nc0_ = t0_ ? c1 : c0, nc1_ = (t1_ ? c0 : c1) + 1;                     \
        v0 = t0_ ? sw0_ : v0;                                                           \
        v1 = t1_ ? sw1_ : st1_;                                                         \
        c0 = nc0_;                                                                      \
        c1 = nc1_;                                                                      \
        if (BT) w |= ((t0_ ? 1ull : 0ull) | (t1_ ? 0ull : 2ull)) << (2 * (J));          \
    }

template <bool CONSTC, bool BT>
__global__ __launch_bounds__(64) void k_rocco_chain(const RoccoJob *__restrict__ jobs, const double *__restrict__ scores,
                                                    const double *__restrict__ costs, const double *__restrict__ pen,
                                                    RoccoRes *__restrict__ res, unsigned long long *bt, unsigned char *sol) {
    constexpr int T = ROCCO_TILE, R = T / 64;
    __shared__ double sS[2][T];
    __shared__ double sC[CONSTC ? 1 : 2][CONSTC ? 1 : T];
    __shared__ unsigned char sSol[BT ? T + 64 : 1];
    const RoccoJob jb = jobs[blockIdx.x];
    const int lane = threadIdx.x;
    const double *s = scores + jb.off;
    const double *cs = CONSTC ? nullptr : costs + jb.off;
    const int64_t n = jb.n, steps = n - 1;      // step q (0 .. n-2) moves from bin q to bin q + 1: score s[q+1], cost cs[q]
    const bool live = lane < jb.nPen;
    const double p = pen[jb.penOff + (live ? lane : 0)];
    double v0 = 0.0, v1 = s[0] - p;
    int c0 = 0, c1 = 1;
    const int64_t nt = (steps + T - 1) / T;
    double rS[R], rC[CONSTC ? 1 : R];
    auto fetch = [&](int64_t t) {
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const int64_t q = t * T + k * 64 + lane;
            rS[k] = q < steps ? s[q + 1] : 0.0;
            if (!CONSTC) rC[k] = q < steps ? cs[q] : 0.0;
        }
    };
    auto stash = [&](int b) {
#pragma unroll
        for (int k = 0; k < R; ++k) {
            sS[b][k * 64 + lane] = rS[k];
            if (!CONSTC) sC[b][k * 64 + lane] = rC[k];
        }
    };
    if (nt > 0) {
        fetch(0);
        stash(0);
    }
    __syncthreads();
    unsigned long long *btc = BT ? bt + jb.off / 32 : nullptr;
    for (int64_t t = 0; t < nt; ++t) {
        const int b = (int)(t & 1);
        if (t + 1 < nt) fetch(t + 1);           // in flight while this tile is walked
        const int cnt = (int)(steps - t * T < T ? steps - t * T : T);
        const double *bs = sS[b];
        const double *bc = CONSTC ? nullptr : sC[b];
        for (int g = 0; g < cnt; g += 32) {
            unsigned long long w = 0ull;
            if (cnt - g >= 32) {
#pragma unroll
                for (int j = 0; j < 32; ++j) CSR_ROCCO_STEP(bs[g + j], CONSTC ? jb.gamma : bc[g + j], j)
            } else {
                for (int j = 0; j < cnt - g; ++j) CSR_ROCCO_STEP(bs[g + j], CONSTC ? jb.gamma : bc[g + j], j)
            }
            if (BT && lane == 0) btc[(t * T + g) >> 5] = w;
        }
        if (t + 1 < nt) stash(b ^ 1);
        __syncthreads();
    }
    // pyx:8697-8704
    const bool f = (v1 > v0) | ((v1 == v0) & (c1 < c0));
    const double bestVal = f ? v1 : v0;
    const int bestCount = f ? c1 : c0;
    if (!BT) {
        if (live) {
            RoccoRes r;
            r.val = bestVal; r.objective = 0.0; r.count = bestCount; r.state = f ? 1 : 0;
            res[jb.penOff + lane] = r;
        }
        return;
    }
    // ---- backtrace (pyx:8706-8714), lane 0: sol[n-1] = final state; sol[k] = bt[state of k+1] recorded by step k
    unsigned char *so = sol + jb.off;
    if (lane == 0) {
        int st = f ? 1 : 0;
        int64_t k = n - 1;
        unsigned long long acc = (unsigned long long)st << (8 * (int)(k & 7));
        if ((k & 7) == 0) { *reinterpret_cast<unsigned long long *>(so + k) = acc; acc = 0ull; }
        if (steps > 0) {
            int64_t wi = (steps - 1) >> 5;
            unsigned long long w = btc[wi];
            for (k = steps - 1; k >= 0; --k) {
                if ((k >> 5) != wi) { wi = k >> 5; w = btc[wi]; }
                st = (int)((w >> (2 * (int)(k & 31) + st)) & 1ull);
                acc |= (unsigned long long)st << (8 * (int)(k & 7));
                if ((k & 7) == 0) { *reinterpret_cast<unsigned long long *>(so + k) = acc; acc = 0ull; }
            }
        }
        __threadfence();
    }
    __syncthreads();
    // ---- unpenalised objective (pyx:8946-8950): the sequential forward sum, lane 0; tiles staged by the wavefront
    double obj = 0.0;
    for (int64_t t0 = 0; t0 < n; t0 += T) {
        const int cnt = (int)(n - t0 < T ? n - t0 : T);
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const int64_t i = t0 + k * 64 + lane;
            sS[0][k * 64 + lane] = i < n ? s[i] : 0.0;
            if (!CONSTC) sC[0][k * 64 + lane] = i < steps ? cs[i] : 0.0;
        }
        for (int k = lane; k < T + 64; k += 64) {
            const int64_t i = t0 + k;
            sSol[k] = i < n ? so[i] : (unsigned char)0;
        }
        __syncthreads();
        if (lane == 0) {
            for (int j = 0; j < cnt; ++j) {
                const unsigned char a = sSol[j];
                obj += sS[0][j] * (double)a;
                if (t0 + j < steps && a != sSol[j + 1]) obj -= CONSTC ? jb.gamma : sC[0][j];
            }
        }
        __syncthreads();
    }
    if (lane == 0) {
        RoccoRes r;
        r.val = bestVal; r.objective = obj; r.count = bestCount; r.state = f ? 1 : 0;
        res[jb.penOff] = r;
    }
}
#undef CSR_ROCCO_STEP

// scoreMin / scoreMax of every chain (pyx:8787-8793).  min and max are associative: any order is exact.
__global__ __launch_bounds__(256) void k_rocco_minmax(const RoccoJob *__restrict__ jobs, const double *__restrict__ scores,
                                                      double *__restrict__ out) {
    __shared__ double sLo[4], sHi[4];
    const RoccoJob jb = jobs[blockIdx.x];
    const double *s = scores + jb.off;
    double lo = s[0], hi = s[0];
    for (int64_t i = threadIdx.x; i < jb.n; i += 256) {
        const double v = s[i];
        lo = v < lo ? v : lo;
        hi = v > hi ? v : hi;
    }
    for (int d = 32; d > 0; d >>= 1) {
        const double a = __shfl_down(lo, d, 64), b = __shfl_down(hi, d, 64);
        lo = a < lo ? a : lo;
        hi = b > hi ? b : hi;
    }
    if ((threadIdx.x & 63) == 0) { sLo[threadIdx.x >> 6] = lo; sHi[threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 4; ++k) {
            lo = sLo[k] < lo ? sLo[k] : lo;
            hi = sHi[k] > hi ? sHi[k] : hi;
        }
        out[2 * blockIdx.x] = lo;
        out[2 * blockIdx.x + 1] = hi;
    }
}

// ---- score track from the resident fit (peaks.py:342-393) ------------------------------------------------------------------
// Pass 1, one workgroup row per chain (blockIdx.y): state mode writes (double) xs0; lower_confidence writes
// raw = (double) xs0 - z * (double)(float) sqrt(Ps00) (the correctly rounded float32 square root) and flags a negative variance.
// Either way the chain's maximum of xs0 goes to mx[chain] (an exact reduction; NaN poisons it like np.max does).
struct RoccoScoreArgs {
    const float *xs, *Ps;       // reference layout: d floats / d*d floats per bin
    int d, lower;               // lower: 1 = lower_confidence
    double z;
    const int64_t *off, *len;   // per chain
    const unsigned char *active;
    double *scores;
    double *mx;                 // nchains, preset to -inf
    int *bad;                   // nchains: a negative variance was seen
};
__device__ __forceinline__ void rocco_atomic_max(double *addr, double v) {
    // (values compared as doubles; a NaN is stored once and then stays)
    unsigned long long *a = reinterpret_cast<unsigned long long *>(addr);
    unsigned long long old = *a;
    for (;;) {
        const double cur = __longlong_as_double((long long)old);
        if (cur != cur || !(v > cur || v != v)) return;
        const unsigned long long seen = atomicCAS(a, old, (unsigned long long)__double_as_longlong(v));
        if (seen == old) return;
        old = seen;
    }
}
__global__ __launch_bounds__(256) void k_rocco_scores(RoccoScoreArgs a) {
    const int ch = blockIdx.y;
    if (a.active && !a.active[ch]) return;
    const int64_t n = a.len[ch], off = a.off[ch];
    double m = -INFINITY;
    bool nan = false;
    int bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float x = a.xs[(off + i) * a.d];
        const double xd = (double)x;
        if (x != x) nan = true;
        m = xd > m ? xd : m;
        double sc = xd;
        if (a.lower) {
            const float v = a.Ps[(off + i) * a.d * a.d];
            const float u = (float)__dsqrt_rn((double)v);     // correctly rounded float32 sqrt (53 >= 2*24+2 bits), = np.sqrt
            if (u < 0.0f || v < 0.0f) bad = 1;
            sc = xd - a.z * (double)u;
        }
        a.scores[off + i] = sc;
    }
    if (nan) m = __longlong_as_double(0x7ff8000000000000ll);
    for (int d = 32; d > 0; d >>= 1) {
        const double o = __shfl_down(m, d, 64);
        m = (o != o || m != m) ? __longlong_as_double(0x7ff8000000000000ll) : (o > m ? o : m);
        bad |= __shfl_down(bad, d, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        rocco_atomic_max(&a.mx[ch], m);
        if (bad) atomicOr(&a.bad[ch], 1);
    }
}
// Pass 2 (lower_confidence): np.maximum(raw, -2 max(xs0)) when that maximum is finite and positive
__global__ __launch_bounds__(256) void k_rocco_floor(RoccoScoreArgs a) {
    const int ch = blockIdx.y;
    if (a.active && !a.active[ch]) return;
    const double mx = a.mx[ch];
    if (!(mx > 0.0) || mx == INFINITY) return;
    const double fl = -2.0 * mx;
    const int64_t n = a.len[ch], off = a.off[ch];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double r = a.scores[off + i];
        a.scores[off + i] = r < fl ? fl : r;
    }
}

// ---- run bounds (pyx:9427-9457): flag -> scan -> compaction ----------------------------------------------------------------
// Bin i starts a run when it is set and no bin of [i - gap - 1, i) is; it ends one when it is set and no bin of
// (i, i + gap + 1] is.  The k-th start and the k-th end belong to the same run.  Counts travel as (starts | ends << 32).
struct RoccoRunArgs {
    const unsigned char *sol;   // one chain
    int64_t n;
    int64_t gap;                // max(maxGapBins, 0), clamped to n
    unsigned long long *blockSum;   // ceil(n / 1024) + 1
    int64_t *starts, *ends;     // capacity entries each (pass 3)
    int64_t capacity;
};
__device__ __forceinline__ unsigned long long rocco_run_flags(const RoccoRunArgs &a, int64_t i) {
    if (i >= a.n || a.sol[i] == 0) return 0ull;
    bool st = true, en = true;
    for (int64_t k = 1; k <= a.gap + 1; ++k) {
        if (i - k >= 0 && a.sol[i - k] != 0) st = false;
        if (i + k < a.n && a.sol[i + k] != 0) en = false;
        if (!st && !en) break;
    }
    return (st ? 1ull : 0ull) | (en ? (1ull << 32) : 0ull);
}
__global__ __launch_bounds__(1024) void k_rocco_run_count(RoccoRunArgs a) {
    __shared__ unsigned long long sh[16];
    const int64_t i = (int64_t)blockIdx.x * 1024 + threadIdx.x;
    unsigned long long total;         // (one scan per launch: wg_scan's barrier in front of its LDS write has nothing to wait for)
    wg_scan<1024>(rocco_run_flags(a, i), sh, total);
    if (threadIdx.x == 1023) a.blockSum[blockIdx.x] = total;
}
__global__ __launch_bounds__(1024) void k_rocco_run_scan(RoccoRunArgs a, int64_t nb) {
    __shared__ unsigned long long sh[16];
    __shared__ unsigned long long carry;
    if (threadIdx.x == 0) carry = 0ull;
    __syncthreads();
    for (int64_t b0 = 0; b0 < nb; b0 += 1024) {
        const int64_t b = b0 + threadIdx.x;
        const unsigned long long v = b < nb ? a.blockSum[b] : 0ull;
        // wg_scan's barrier stands in front of its write of sh, so the next round's call waits for this round's reads of sh; no
        // barrier is needed behind the scan.  carry keeps its own two: read by all, barrier, written by one, barrier
        unsigned long long total;
        const unsigned long long inc = wg_scan<1024>(v, sh, total);
        const unsigned long long c = carry;
        if (b < nb) a.blockSum[b] = c + inc - v;        // exclusive
        __syncthreads();
        if (threadIdx.x == 1023) carry = c + total;
        __syncthreads();
    }
    if (threadIdx.x == 0) a.blockSum[nb] = carry;
}
__global__ __launch_bounds__(1024) void k_rocco_run_write(RoccoRunArgs a) {
    __shared__ unsigned long long sh[16];
    const int64_t i = (int64_t)blockIdx.x * 1024 + threadIdx.x;
    const unsigned long long fl = rocco_run_flags(a, i);
    unsigned long long total;         // (one scan per launch, as in k_rocco_run_count)
    const unsigned long long ex = wg_scan<1024>(fl, sh, total) - fl + a.blockSum[blockIdx.x];
    const int64_t ks = (int64_t)(ex & 0xffffffffull), ke = (int64_t)(ex >> 32);
    if ((fl & 1ull) && ks < a.capacity) a.starts[ks] = i;
    if ((fl >> 32) && ke < a.capacity) a.ends[ke] = i;
}

}  // namespace csr
