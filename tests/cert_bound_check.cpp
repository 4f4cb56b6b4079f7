// cert_bound_check.cpp — CPU check of rag_project_icd10_amd/csrc/cert_bound.hpp (plain C++, built by
// tests/test_tight_bound_cpu.py with g++ under ASan + UBSan): the header's fp32 arithmetic never comes out below the same
// expression in long double, over a sweep of norms from 2^-30 to 2^30 and the dims the fp16 path exists for.
#include <cmath>
#include <cstdio>
#include <random>

#include "cert_bound.hpp"

int main() {
    using namespace icd;
    long checks = 0;
    const int dims[] = {768, 1024};
    for (int dim : dims) {
        const float acc = cert_acc_rel(dim);
        const long double acc_min = 3.0L * dim * ldexpl(1.0L, -24) * (1.0L + ldexpl(1.0L, -9)) + ldexpl(1.0L, -22);
        if (!((long double)acc >= acc_min)) { printf("FAIL acc_rel dim %d: %.9g < %.9Lg\n", dim, acc, acc_min); return 1; }
        // the two chains this weight pays for: D 2^-23 (MFMA, any internal rounding) + gamma_D of the fmaf chain
        const long double u = ldexpl(1.0L, -24), chains = 2.0L * dim * u + dim * u / (1.0L - dim * u);
        if (!(acc_min - ldexpl(1.0L, -22) >= chains)) { printf("FAIL chains dim %d\n", dim); return 1; }
        ++checks;
        std::mt19937_64 rng(12345u + dim);
        std::uniform_real_distribution<double> mant(1.0, 2.0), rel(1e-5, 1e-3);
        std::uniform_int_distribution<int> ex(-30, 30);
        for (int i = 0; i < 200000; ++i) {
            const float qn = (float)ldexp(mant(rng), ex(rng)), cmax = (float)ldexp(mant(rng), ex(rng));
            const float qres = (float)(qn * rel(rng)), dcmax = (float)(cmax * rel(rng));
            const float c16 = cert_cmax16(cmax, dcmax);
            if (!((long double)c16 >= (long double)cmax + dcmax)) { printf("FAIL cmax16 %.9g %.9g\n", cmax, dcmax); return 1; }
            const float e = cert_eps_round(qn, qres, c16, dcmax, acc);
            const long double want = (long double)qres * c16 + (long double)qn * dcmax + (long double)acc * (((long double)qn + qres) * c16);
            if (!((long double)e >= want) || !std::isfinite(e)) { printf("FAIL eps %.9g < %.9Lg (qn %.9g qres %.9g c16 %.9g dc %.9g)\n", e, want, qn, qres, c16, dcmax); return 1; }
            // ... and it stays a tight bound: the upward margins are a few 2^-18
            if (!((long double)e <= want * (1.0L + ldexpl(1.0L, -16)))) { printf("FAIL eps loose %.9g %.9Lg\n", e, want); return 1; }
            checks += 3;
        }
    }
    printf("%ld checks ok\n", checks);
    return 0;
}
