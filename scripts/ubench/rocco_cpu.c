// rocco_cpu.c -- the CPU column of scripts/rocco_bench.py: this project's own plain-C restatement of the sequential ROCCO
// algorithm (two-state chain DP with backtrace inside a count-driven bisection of the selection penalty, then the
// unpenalised objective), one chain after the other on ONE core.  Built by the script with the flags the reference's
// extension is built with (-O3 -fno-trapping-math -fno-math-errno -mtune=generic) plus -ffp-contract=off:
//   gcc -O3 -fno-trapping-math -fno-math-errno -mtune=generic -ffp-contract=off -shared -fPIC -o librocco_cpu.so rocco_cpu.c -lm
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct { double val; int64_t count; } res_t;

static res_t solve(const double *s, int64_t n, double gamma, double p, uint8_t *bt0, uint8_t *bt1, uint8_t *sol) {
    res_t r;
    if (n == 1) {
        const double v = s[0] - p;
        sol[0] = v > 0.0;
        r.val = v > 0.0 ? v : 0.0;
        r.count = v > 0.0;
        return r;
    }
    double v0 = 0.0, v1 = s[0] - p;
    int64_t c0 = 0, c1 = 1;
    for (int64_t i = 1; i < n; ++i) {
        double n0v, n1v;
        int64_t n0c, n1c;
        const double sw0 = v1 - gamma;
        if (sw0 > v0 || (sw0 == v0 && c1 < c0)) { n0v = sw0; n0c = c1; bt0[i] = 1; } else { n0v = v0; n0c = c0; bt0[i] = 0; }
        const double st1 = v1 + s[i] - p, sw1 = v0 - gamma + s[i] - p;
        if (sw1 > st1 || (sw1 == st1 && c0 + 1 < c1 + 1)) { n1v = sw1; n1c = c0 + 1; bt1[i] = 0; } else { n1v = st1; n1c = c1 + 1; bt1[i] = 1; }
        v0 = n0v; c0 = n0c; v1 = n1v; c1 = n1c;
    }
    int state;
    if (v1 > v0 || (v1 == v0 && c1 < c0)) { r.val = v1; r.count = c1; state = 1; } else { r.val = v0; r.count = c0; state = 0; }
    sol[n - 1] = (uint8_t)state;
    for (int64_t i = n - 1; i > 0; --i) {
        state = state == 0 ? bt0[i] : bt1[i];
        sol[i - 1] = (uint8_t)state;
    }
    return r;
}

// out: penalty, penalised objective, objective, count (as double); sol: n bytes.  Returns the number of chain passes made.
int64_t rocco_chrom(const double *s, int64_t n, double budget, double gamma, int max_iter, double *out, uint8_t *sol) {
    uint8_t *bt0 = malloc((size_t)n), *bt1 = malloc((size_t)n), *tmp = malloc((size_t)n);
    int64_t target = (int64_t)floor((double)n * budget), passes = 0;
    if (target < 0) target = 0;
    if (target > n) target = n;
    double pen;
    res_t best;
    if (target == n) {
        pen = 0.0;
        best = solve(s, n, gamma, 0.0, bt0, bt1, sol);
        ++passes;
    } else {
        double lo = s[0], hi = s[0], ssum = 0.0;
        for (int64_t i = 0; i < n; ++i) {
            if (s[i] < lo) lo = s[i];
            if (s[i] > hi) hi = s[i];
            if (i < n - 1) ssum += gamma;
        }
        double lower = lo - ssum - 1.0, upper = hi + ssum + 1.0;
        res_t l = solve(s, n, gamma, lower, bt0, bt1, tmp);
        ++passes;
        while (l.count <= target) { lower -= fmax(1.0, fabs(lower)); l = solve(s, n, gamma, lower, bt0, bt1, tmp); ++passes; }
        best = solve(s, n, gamma, upper, bt0, bt1, sol);
        ++passes;
        while (best.count > target) { upper += fmax(1.0, fabs(upper)); best = solve(s, n, gamma, upper, bt0, bt1, sol); ++passes; }
        const int it = max_iter > 1 ? max_iter : 1;
        for (int k = 0; k < it; ++k) {
            const double mid = (lower + upper) / 2.0;
            const res_t r = solve(s, n, gamma, mid, bt0, bt1, tmp);
            ++passes;
            if (r.count > target) lower = mid;
            else { upper = mid; best = r; memcpy(sol, tmp, (size_t)n); }
        }
        pen = upper;
    }
    double obj = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        obj += s[i] * (double)sol[i];
        if (i < n - 1 && sol[i] != sol[i + 1]) obj -= gamma;
    }
    out[0] = pen; out[1] = best.val; out[2] = obj; out[3] = (double)best.count;
    free(bt0); free(bt1); free(tmp);
    return passes;
}
