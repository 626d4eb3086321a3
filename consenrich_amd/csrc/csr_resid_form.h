// csr_resid_form.h -- which residual kernel serves a batch of m samples, with how much LDS, and in which slabs of sample rows
// (launch_resid / launch_resid_runs, csr_host_pipeline.inl; resid_dev / resid_v4_dev<K>, csr_device.h).  Plain C++17, no headers
// at all: tests/resid_form_check.cpp compiles it without HIP, and the kernels read the same slab constants.
//
// A workgroup stages K * 64 bins x `rows` sample rows in LDS, each row padded (1 float in the plain form, 4 in the 16-byte form so
// that float4 rows stay 16-byte aligned).  Up to the slab length all m rows are staged at once -- one slab, the form every batch
// had while nothing bounded m.  Past it the kernel walks the rows in slabs of that length (the last one shorter), so the LDS
// request never exceeds 64 KB: no launch attribute is needed and no m is refused.
#pragma once

constexpr int RESID_LDS_MAX = 65536;                 // bytes: what a kernel may request without a launch attribute
constexpr int resid_row_bytes(bool v4, int K) { return (int)sizeof(float) * (K * 64 + (v4 ? 4 : 1)); }
// sample rows of one slab: all that fit RESID_LDS_MAX, a multiple of 4 in the 16-byte form (its stores cover 4 samples)
constexpr int resid_slab_rows(bool v4, int K) {
    return v4 ? RESID_LDS_MAX / resid_row_bytes(true, K) / 4 * 4 : RESID_LDS_MAX / resid_row_bytes(false, 1);
}
constexpr int RESID_SLAB_PLAIN = resid_slab_rows(false, 1);      // 252 rows of 260 bytes
constexpr int RESID_SLAB_V4_K1 = resid_slab_rows(true, 1);       // 240 rows of 272 bytes
constexpr int RESID_SLAB_V4_K2 = resid_slab_rows(true, 2);       // 124 rows of 528 bytes: K = 2 is chosen up to here only
static_assert(RESID_SLAB_PLAIN == 252 && RESID_SLAB_V4_K1 == 240 && RESID_SLAB_V4_K2 == 124, "slab lengths");

// The form for m samples: the 16-byte form (m a multiple of 4) with K = 2 (measured best: 0.665 vs 0.684 ms with 1 or 4, round
// 3) while its whole tile fits 64 KB, else with K = 1; the plain form otherwise.  `slab` rows at a time, `lds` bytes.
struct ResidForm { bool v4; int K; int slab; int lds; };
constexpr ResidForm resid_form(int m) {
    const bool v4 = (m & 3) == 0;
    const int K = v4 && m <= RESID_SLAB_V4_K2 ? 2 : 1;
    const int slab = resid_slab_rows(v4, K);
    return ResidForm{v4, K, slab, resid_row_bytes(v4, K) * (m < slab ? m : slab)};
}
// the slabs of a form: rows [resid_slab_begin(f, s), + resid_slab_len(f, m, s)) for s in [0, resid_slab_count(f, m))
constexpr int resid_slab_count(const ResidForm &f, int m) { return (m + f.slab - 1) / f.slab; }
constexpr int resid_slab_begin(const ResidForm &f, int s) { return s * f.slab; }
constexpr int resid_slab_len(const ResidForm &f, int m, int s) { return m - s * f.slab < f.slab ? m - s * f.slab : f.slab; }
