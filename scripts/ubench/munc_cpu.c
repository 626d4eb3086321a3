/* munc_cpu.c -- a plain-C restatement, written from scratch, of the two dense observation-variance seed natives the device runs
 * (csrc/csr_munc.h): the observation-moment seed pass and the rolling mean of the local evidence.  One core, no threads: the CPU
 * yardstick of scripts/munc_seed_bench.py, and checked bit for bit against the compiled reference's fixtures by
 * tests/test_munc_twin.py.
 *
 *     gcc -O3 -fno-trapping-math -fno-math-errno -mtune=generic -ffp-contract=off -shared -fPIC -o libmunc_cpu.so munc_cpu.c
 *
 * Masks: mode 0 none, 1 per interval, 2 per cell; nonzero = active in the seed pass, excluded in the rolling mean.
 * Both return 0, or 1 when an active cell is invalid (nothing useful has been written then). */
#include <math.h>
#include <stddef.h>
#include <stdint.h>

static int mask_set(const uint8_t *mask, int mode, long n, long j, long k) { return mode == 1 ? mask[k] != 0 : mask[j * n + k] != 0; }

static void cascade(double *local, double *total, double count, double floor_, double cap) {
    if (*local < floor_) *local = floor_;
    *total = *local + count;
    if (*total > cap) {
        *total = cap;
        *local = *total - count;
        if (*local < floor_) {
            *local = floor_;
            *total = *local + count;
        }
    }
}

int munc_cpu_seed_pass(long m, long n, const float *data, const float *munc, const float *mean, const float *var, const float *bg,
                       const float *gvar, const float *cfloor, const float *omega_in, const float *rho_in, const uint8_t *active,
                       int mode, double pad, double ds, double d_omega, double omega_min, double omega_max, double floor_, double cap,
                       int weighted, int update, float *moment, float *rho_out, float *omega_raw, float *omega_out, float *local,
                       float *variance) {
    for (long k = 0; k < n; ++k) {
        const double state = mean[k], b = bg ? bg[k] : 0.0;
        double base = var[k];
        int bad_k = !isfinite(state) || !isfinite(base) || !isfinite(b);
        if (gvar) {
            bad_k = bad_k || !isfinite((double)gvar[k]);
            base += gvar[k];
        }
        if (base < 0.0) base = 0.0;
        double om_in = 1.0, omega = 1.0, raw = 1.0;
        if (weighted && omega_in) {
            om_in = omega_in[k];
            bad_k = bad_k || !isfinite(om_in) || om_in <= 0.0;
        }
        if (weighted && update) {
            double dbar = 0.0;
            long cnt = 0;
            for (long j = 0; j < m; ++j) {
                const long i = j * n + k;
                if (mode && !mask_set(active, mode, n, j, k)) {
                    moment[i] = 0.0f;
                    rho_out[i] = 1.0f;
                    continue;
                }
                double bv = (double)munc[i] + pad;
                if (bad_k || !isfinite((double)data[i]) || !isfinite(bv) || bv <= 0.0) return 1;
                if (bv < floor_) bv = floor_;
                const double r = (double)data[i] - b - state, mo = r * r + base;
                moment[i] = (float)mo;
                rho_out[i] = (float)((ds + 1.0) / (ds + om_in * mo / bv));
                dbar += mo / bv;
                ++cnt;
            }
            if (cnt > 0) {
                dbar = dbar / (double)cnt;
                raw = (d_omega + 1.0) / (d_omega + dbar);
                omega = raw < omega_min ? omega_min : (raw > omega_max ? omega_max : raw);
            }
        } else if (weighted) {
            raw = om_in;
            omega = raw < omega_min ? omega_min : (raw > omega_max ? omega_max : raw);
        }
        omega_raw[k] = (float)raw;
        omega_out[k] = (float)omega;
        for (long j = 0; j < m; ++j) {
            const long i = j * n + k;
            const double count = cfloor ? cfloor[i] : 0.0;
            double lv, tv;
            if (mode && !mask_set(active, mode, n, j, k)) {
                lv = (double)munc[i] - count;
                moment[i] = 0.0f;
                rho_out[i] = 1.0f;
            } else {
                if (bad_k || (cfloor && (!isfinite(count) || count < 0.0))) return 1;
                if (!(weighted && update)) {
                    const double bv = (double)munc[i] + pad, r = (double)data[i] - b - state;
                    if (!isfinite((double)data[i]) || !isfinite(bv) || bv <= 0.0) return 1;
                    const float rin = weighted ? (rho_in ? rho_in[i] : 1.0f) : 1.0f;
                    if (weighted && (!isfinite((double)rin) || rin <= 0.0f)) return 1;
                    moment[i] = (float)(r * r + base);
                    rho_out[i] = rin;
                    lv = weighted ? 0.0 : r * r + base - pad - count;
                }
                if (weighted) lv = omega * (double)rho_out[i] * (double)moment[i] - pad - count;
            }
            cascade(&lv, &tv, count, floor_, cap);
            local[i] = (float)lv;
            variance[i] = (float)tv;
        }
    }
    return 0;
}

int munc_cpu_smooth(long m, long n, const float *local, long window, const uint8_t *exclude, int mode, double eps, float *out) {
    const long half = window / 2;
    for (long j = 0; j < m; ++j)
        for (long i = 0; i < n; ++i) {
            if (mode && mask_set(exclude, mode, n, j, i)) continue;
            const double v = local[j * n + i];
            if (!isfinite(v) || v <= 0.0) return 1;
        }
    for (long j = 0; j < m; ++j) {
        const float *row = local + j * n;
        long left = 0, right = 0, count = 0;
        double sum = 0.0;
        for (long i = 0; i < n; ++i) {
            long tl = i >= half ? i - half : 0, tr = tl + window;
            if (tr > n) {
                tr = n;
                tl = tr >= window ? tr - window : 0;
            }
            for (; right < tr; ++right)
                if (!(mode && mask_set(exclude, mode, n, j, right))) {
                    sum += (double)row[right];
                    ++count;
                }
            for (; left < tl; ++left)
                if (!(mode && mask_set(exclude, mode, n, j, left))) {
                    sum -= (double)row[left];
                    --count;
                }
            double v = count > 0 ? sum / (double)count : (double)row[i];
            if (v < eps) v = eps;
            out[j * n + i] = (float)v;
        }
    }
    return 0;
}
