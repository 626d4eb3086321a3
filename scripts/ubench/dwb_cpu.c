// dwb_cpu.c -- the CPU column of scripts/dwb_bench.py: this project's own plain-C restatement of one stationary-null DWB draw
// (a (2 maxLag + 1)-tap moving sum of the noise with Bartlett weights, standardised by its own mean and sd, multiplied into
// the template and re-centred), every sum in index order, on ONE core.  Built by the script with the flags the reference's
// extension is built with plus -ffp-contract=off:
//   gcc -O3 -fno-trapping-math -fno-math-errno -mtune=generic -ffp-contract=off -shared -fPIC -o libdwb_cpu.so dwb_cpu.c -lm
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

// noise: n + 2 bw values; out: n values.  Returns 0, or -1 when memory runs out.
int dwb_draw_bartlett(const double *tmpl, int64_t n, int bandwidth, const double *noise, double *out) {
    const int bw = bandwidth >= 2 ? bandwidth : 2, taps = 2 * bw + 1;
    double *w = (double *)malloc(sizeof(double) * (size_t)taps);
    if (!w) return -1;
    double normSq = 0.0;
    for (int j = 0; j < taps; ++j) {
        const double ax = fabs((double)(j - bw)) / (double)bw;
        w[j] = ax <= 1.0 ? 1.0 - ax : 0.0;
        normSq += w[j] * w[j];
    }
    const double norm = sqrt(fmax(normSq, DBL_MIN));
    for (int j = 0; j < taps; ++j) w[j] = w[j] / norm;
    double mean = 0.0, var = 0.0, sd = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        double v = 0.0;
        for (int j = 0; j < taps; ++j) v += noise[i + j] * w[j];
        out[i] = v;
        mean += v;
    }
    mean = mean / (double)n;
    if (n >= 2) {
        for (int64_t i = 0; i < n; ++i) {
            const double d = out[i] - mean;
            var += d * d;
        }
        sd = sqrt(var / (double)(n - 1));
    }
    const int flat = !isfinite(sd) || sd <= DBL_MIN;
    double m2 = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        out[i] = tmpl[i] * (flat ? 1.0 : (out[i] - mean) / sd);
        m2 += out[i];
    }
    m2 = m2 / (double)n;
    for (int64_t i = 0; i < n; ++i) out[i] = out[i] - m2;
    free(w);
    return 0;
}
