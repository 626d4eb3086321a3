// ess_cpu.c -- the positive-autocorrelation effective sample size scan as a caller without the device path would run it: plain C,
// one core, the fast path (no mask, no log, no window).  The CPU column of scripts/budget_bench.py.
//
//     cc -O3 -ffp-contract=off -shared -fPIC -o libess_cpu.so ess_cpu.c
//
// Every sum runs in index order with a separate multiply and add, so the result is the one the device path returns, bit for bit.
// x is centred in place.  out = {n_eff, tau, lags_used}.
#include <math.h>

void ess_cpu(double *x, long n, long max_lag, double *out) {
    out[0] = (double)n;
    out[1] = 1.0;
    out[2] = 0.0;
    if (n < 2) return;
    double mean = 0.0, var = 0.0;
    for (long i = 0; i < n; ++i) mean += x[i];
    mean /= (double)n;
    for (long i = 0; i < n; ++i) {
        x[i] = x[i] - mean;
        var += x[i] * x[i];
    }
    var /= (double)n;
    if (!isfinite(var) || var <= 2.2250738585072014e-308) return;
    long last = max_lag < n - 1 ? max_lag : n - 1;
    if (last < 1) last = 1;
    double tau = 1.0;
    long used = 0;
    for (long lag = 1; lag <= last; ++lag) {
        double cov = 0.0;
        for (long i = 0; i < n - lag; ++i) cov += x[i] * x[i + lag];
        cov /= (double)(n - lag > 1 ? n - lag : 1);
        const double rho = cov / var;
        if (!isfinite(rho) || rho <= 0.0) break;
        tau += 2.0 * rho;
        used = lag;
    }
    if (tau < 1.0) tau = 1.0;
    out[0] = (double)n / tau;
    out[1] = tau;
    out[2] = (double)used;
}
