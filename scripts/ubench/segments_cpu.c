// segments_cpu.c -- the CPU column of scripts/segments_bench.py: this project's own plain-C restatement of the multiscale
// candidate-segment stage (per scale: prefix of the track and the centred moving mean; per (scale, view): the excess and its
// prefix, runs of smooth > threshold bridged over at most `gap` false bins, the minRun filter, integrated / mean / score / max
// per run), one (scale, view) after the other on ONE core, with the passes over the track the sequential formulation makes
// (the prefix again for every scale, the excess again for every (scale, view)).  It returns every candidate; the per-view cap --
// two NumPy calls in the original -- is applied by the script.  Built by the script with the flags the reference's extension is
// built with (-O3 -fno-trapping-math -fno-math-errno -mtune=generic) plus -ffp-contract=off:
//   gcc -O3 -fno-trapping-math -fno-math-errno -mtune=generic -ffp-contract=off -shared -fPIC -o libsegments_cpu.so segments_cpu.c -lm
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

// Rows go to the output arrays while they fit `capacity`; the return value is the number of rows there are (call again with
// more room if it is larger), or -1 when memory runs out.  view_count[scale * n_views + view] = candidates of that view.
int64_t segments_cpu(const double *x, int64_t n, const int64_t *scales, int32_t n_scales, const double *thresholds,
                     const double *null_scales, int32_t n_views, int32_t min_run_bins, int32_t max_gap_bins, int64_t capacity,
                     int64_t *start, int64_t *end, double *score, double *integrated, double *mean, double *max_excess,
                     int64_t *view_count) {
    const int64_t min_run = min_run_bins > 1 ? min_run_bins : 1, gap = max_gap_bins > 0 ? max_gap_bins : 0;
    int64_t rows = 0;
    if (n <= 0 || n_scales <= 0 || n_views <= 0) return 0;
    double *prefix = malloc(sizeof(double) * (size_t)(n + 1)), *smooth = malloc(sizeof(double) * (size_t)n);
    double *excess = malloc(sizeof(double) * (size_t)n), *ex_prefix = malloc(sizeof(double) * (size_t)(n + 1));
    if (!prefix || !smooth || !excess || !ex_prefix) {
        free(prefix); free(smooth); free(excess); free(ex_prefix);
        return -1;
    }
    for (int32_t si = 0; si < n_scales; ++si) {
        int64_t w = scales[si];
        if (w < 1) w = 1;
        if (w > n) w = n;
        prefix[0] = 0.0;
        for (int64_t i = 0; i < n; ++i) prefix[i + 1] = prefix[i] + x[i];
        if (w <= 1 || n <= 1) {
            for (int64_t i = 0; i < n; ++i) smooth[i] = x[i];
        } else {
            const int64_t left = (w - 1) / 2, right = w - 1 - left;
            for (int64_t i = 0; i < n; ++i) {
                const int64_t a = i - left < 0 ? 0 : i - left, b = i + right + 1 > n ? n : i + right + 1;
                smooth[i] = (prefix[b] - prefix[a]) / (double)w;
            }
        }
        for (int32_t vi = 0; vi < n_views; ++vi) {
            const double thr = thresholds[vi];
            double ns = null_scales[vi];
            if (ns < DBL_MIN) ns = DBL_MIN;
            ex_prefix[0] = 0.0;
            for (int64_t i = 0; i < n; ++i) {
                double v = (x[i] - thr) / ns;
                if (v < 0.0) v = 0.0;
                excess[i] = v;
                ex_prefix[i + 1] = ex_prefix[i] + v;
            }
            int64_t kept = 0, run_start = -1, last = -1;
            for (int64_t i = 0; i <= n; ++i) {
                const int on = i < n && smooth[i] > thr;
                const int close = run_start >= 0 && (i == n || (on && i - last > gap + 1));
                if (close) {
                    const int64_t len = last - run_start + 1;
                    if (len >= min_run) {
                        if (rows < capacity) {
                            const double integ = ex_prefix[last + 1] - ex_prefix[run_start];
                            double m = 0.0;
                            for (int64_t j = run_start; j <= last; ++j)
                                if (excess[j] > m) m = excess[j];
                            start[rows] = run_start;
                            end[rows] = last;
                            integrated[rows] = integ;
                            mean[rows] = integ / (double)len;
                            score[rows] = integ / sqrt(fmax((double)len, 1.0));
                            max_excess[rows] = m;
                        }
                        ++rows;
                        ++kept;
                    }
                    run_start = -1;
                }
                if (on) {
                    if (run_start < 0) run_start = i;
                    last = i;
                }
            }
            view_count[(int64_t)si * n_views + vi] = kept;
        }
    }
    free(prefix); free(smooth); free(excess); free(ex_prefix);
    return rows;
}
