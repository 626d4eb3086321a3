// shrink_cpu.c -- one EM pass and the posterior pass of the state shrinkage as a caller without the device path would run them:
// plain C, one core, every sum bin after bin.  The CPU column of scripts/shrink_bench.py.
//
//     cc -O3 -ffp-contract=off -shared -fPIC -o libshrink_cpu.so shrink_cpu.c -lm
//
// The arithmetic is that of csrc/csr_shrink.h (and of tests/twin_shrink.py `SequentialPasses`): a bin is valid iff x and v are
// finite and v > 0, a valid variance at or below 1e-12 counts as 1e-12, a valid bin weighs 1 / (valid bins of its block), K slabs
// with variances tau and log prior weights lsp.  K <= 96.
//   shrink_cpu_em    out = {totalWeight, nullMass, logLikelihood, finiteCount, slabMass[K], slabSecond[K]}
//   shrink_cpu_post  out = five float tracks of n values: shrunk, posterior sd, spike probability, slab mean, slab weight
#include <math.h>

#define TWO_PI (2.0 * 3.14159265358979323846)
#define FLOOR 1.0e-12
#define MAX_K 96

static int valid(double x, double v) { return isfinite(x) && isfinite(v) && v > 0.0; }

void shrink_cpu_em(const double *x, const double *v, long n, long block, double pi0, int K, const double *tau, const double *lsp,
                   double *out) {
    double e[MAX_K];
    const double logNullPrior = log(pi0);
    for (int q = 0; q < 4 + 2 * K; ++q) out[q] = 0.0;
    for (long start = 0; start < n; start += block) {
        const long end = start + block < n ? start + block : n;
        long cnt = 0;
        for (long i = start; i < end; ++i) cnt += valid(x[i], v[i]);
        if (cnt == 0) continue;
        const double weight = 1.0 / (double)cnt;
        for (long i = start; i < end; ++i) {
            if (!valid(x[i], v[i])) continue;
            const double xi = x[i], vi = v[i] <= FLOOR ? FLOOR : v[i], x2 = xi * xi;
            const double logNull = logNullPrior - 0.5 * (log(TWO_PI * vi) + x2 / vi);
            double maxLog = logNull;
            for (int j = 0; j < K; ++j) {
                const double vt = vi + tau[j];
                e[j] = lsp[j] - 0.5 * (log(TWO_PI * vt) + x2 / vt);
                if (e[j] > maxLog) maxLog = e[j];
            }
            const double e0 = exp(logNull - maxLog);
            double denom = e0;
            for (int j = 0; j < K; ++j) {
                e[j] = exp(e[j] - maxLog);
                denom += e[j];
            }
            out[0] += weight;
            out[1] += weight * (e0 / denom);
            out[2] += weight * (maxLog + log(denom));
            out[3] += 1.0;
            for (int j = 0; j < K; ++j) {
                const double resp = e[j] / denom, s = tau[j] / (tau[j] + vi), mean = s * xi;
                out[4 + j] += weight * resp;
                out[4 + K + j] += weight * resp * (s * vi + mean * mean);
            }
        }
    }
}

void shrink_cpu_post(const double *x, const double *v, long n, double pi0, int K, const double *tau, const double *lsp, float *out) {
    double e[MAX_K];
    const double logNullPrior = log(pi0);
    float *shrunkT = out, *sdT = out + n, *spikeT = out + 2 * n, *meanT = out + 3 * n, *weightT = out + 4 * n;
    for (long i = 0; i < n; ++i) {
        if (!valid(x[i], v[i])) {
            shrunkT[i] = (float)x[i];
            sdT[i] = spikeT[i] = meanT[i] = weightT[i] = NAN;
            continue;
        }
        const double xi = x[i], vi = v[i] <= FLOOR ? FLOOR : v[i], x2 = xi * xi;
        const double logNull = logNullPrior - 0.5 * (log(TWO_PI * vi) + x2 / vi);
        double maxLog = logNull;
        for (int j = 0; j < K; ++j) {
            const double vt = vi + tau[j];
            e[j] = lsp[j] - 0.5 * (log(TWO_PI * vt) + x2 / vt);
            if (e[j] > maxLog) maxLog = e[j];
        }
        const double e0 = exp(logNull - maxLog);
        double denom = e0;
        for (int j = 0; j < K; ++j) {
            e[j] = exp(e[j] - maxLog);
            denom += e[j];
        }
        double shrunk = 0.0, second = 0.0, w = 0.0;
        for (int j = 0; j < K; ++j) {
            const double resp = e[j] / denom, s = tau[j] / (tau[j] + vi), mean = s * xi;
            w += resp;
            shrunk += resp * mean;
            second += resp * (s * vi + mean * mean);
        }
        double var = second - shrunk * shrunk;
        if (!isfinite(var) || var <= FLOOR) var = FLOOR;
        shrunkT[i] = (float)shrunk;
        sdT[i] = (float)sqrt(var);
        spikeT[i] = (float)(e0 / denom);
        meanT[i] = w > FLOOR ? (float)(shrunk / w) : 0.0f;
        weightT[i] = (float)w;
    }
}
