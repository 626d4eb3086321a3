// Stand-alone check of consenrich_amd/csrc/csr_resid_form.h (tests/test_abi_and_host.py compiles it with
// g++ -std=c++17 -fsanitize=address,undefined and runs it): for every sample count the gain summary admits (1 .. 65535) the
// residual kernels' LDS request stays within 64 KB and their slabs of sample rows tile [0, m) exactly; where the whole tile fits
// 64 KB the form is the one-slab form the kernels had before slabs existed.  No HIP, no GPU.
#include "csr_resid_form.h"

#include <cstdio>
#include <cstdlib>

#define REQUIRE(cond)                                                              \
    do {                                                                           \
        if (!(cond)) { fprintf(stderr, "%s:%d: %s (m = %d)\n", __FILE__, __LINE__, #cond, m); exit(1); } \
    } while (0)

// the form written out independently: bytes of one staged row, and the unbounded request of the kernels before slabs
static long row_bytes(bool v4, int K) { return 4L * (K * 64 + (v4 ? 4 : 1)); }

static void check_slabs(int m) {
    const ResidForm f = resid_form(m);
    REQUIRE(f.v4 == (m % 4 == 0));
    REQUIRE(f.K == 1 || (f.K == 2 && f.v4));
    REQUIRE(f.lds > 0 && f.lds <= 65536);
    REQUIRE(f.slab > 0 && (!f.v4 || f.slab % 4 == 0));
    const int count = resid_slab_count(f, m);
    REQUIRE(count >= 1);
    // every row exactly once: each slab starts where the one before it ended, the last ends at m; every slab fits the request
    int next = 0;
    for (int s = 0; s < count; ++s) {
        const int b = resid_slab_begin(f, s), len = resid_slab_len(f, m, s);
        REQUIRE(b == next && len > 0 && b + len <= m);
        REQUIRE(row_bytes(f.v4, f.K) * len <= f.lds);
        if (f.v4) REQUIRE(b % 4 == 0 && len % 4 == 0);
        next = b + len;
    }
    REQUIRE(next == m);
    // the request is no larger than the longest slab needs
    REQUIRE(f.lds == row_bytes(f.v4, f.K) * resid_slab_len(f, m, 0));
    // K = 2 never walks slabs (the kernel stages all m rows for it)
    if (f.K == 2) REQUIRE(count == 1);
    // wherever the one-slab form fits 64 KB it IS the form: K = 2 up to 528 m <= 65536, then K = 1; the plain form otherwise
    const bool v4 = m % 4 == 0;
    const int K = v4 && 528L * m <= 65536 ? 2 : 1;
    const long whole = row_bytes(v4, K) * m;
    if (whole <= 65536) REQUIRE(count == 1 && f.v4 == v4 && f.K == K && f.lds == whole);
    else REQUIRE(count >= 2 && f.K == 1);
}

struct Row { int m; bool v4; int K; int lds; };

int main() {
    int m = 0;
    for (m = 1; m <= 65535; ++m) check_slabs(m);
    // the literal table: form, K and bytes at the edges of each form
    const Row table[] = {{4, true, 2, 528 * 4},     {124, true, 2, 528 * 124}, {125, false, 1, 260 * 125},
                         {128, true, 1, 272 * 128}, {240, true, 1, 272 * 240}, {251, false, 1, 260 * 251}};
    for (const Row &r : table) {
        m = r.m;
        const ResidForm f = resid_form(m);
        REQUIRE(f.v4 == r.v4 && f.K == r.K && f.lds == r.lds && resid_slab_count(f, m) == 1);
    }
    REQUIRE(528 * 124 == 65472 && 272 * 240 == 65280 && 260 * 251 == 65260);
    // past the one-slab forms: bounded, several slabs
    const int past[] = {244, 252, 253, 256, 604, 631};
    for (int v : past) {
        m = v;
        const ResidForm f = resid_form(m);
        REQUIRE(f.lds <= 65536 && f.K == 1 && resid_slab_count(f, m) >= 2);
    }
    m = 244;
    REQUIRE(resid_slab_count(resid_form(m), m) == 2 && resid_slab_len(resid_form(m), m, 1) == 4);
    m = 253;
    REQUIRE(resid_slab_count(resid_form(m), m) == 2 && resid_slab_len(resid_form(m), m, 1) == 1);
    m = 631;
    REQUIRE(resid_slab_count(resid_form(m), m) == 3 && resid_slab_len(resid_form(m), m, 2) == 631 - 2 * 252);
    printf("resid_form_check ok\n");
    return 0;
}
