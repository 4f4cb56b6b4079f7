// cert_bound.hpp — the error bound of finalize's certificate: plain C++, shared by the kernel
// (finalize.hpp, fin_eps), by icd_index_create and by the CPU checker tests/cert_bound_check.cpp.
//
// Everything is in the coarse pass's SCALED units 2^(qexp + cexp). q' and c' are the scaled fp32 query and corpus row (the
// centred row when the image is centred), q16 and c16 their fp16 images, dq = q16 - q', dc = c16 - c'. In exact arithmetic
//     q16.c16 - q'.c' = dq.c16 + q'.dc,   so   |q16.c16 - q'.c'| <= |dq| |c16| + |q'| |dc|       (Cauchy-Schwarz)
// convert_rows_kernel measures |dq| per query and the maximum of |dc| over the corpus while it rounds the rows (each
// component's residual x - fp16(x) is exact in fp32), so neither factor is a worst case of the format any more. On top come
//   * the two summations: the MFMA chain of the coarse score (D products; ASSUMED, not measured: the matrix unit adds each
//     with a relative error of at most 2^-23, twice an fp32 rounding, whatever its internal multi-operand adder does - the
//     former constant 1.2e-3 carried the same allowance) and the canonical fp32 fmaf chain (gamma_D = D 2^-24 / (1 - D 2^-24)), both
//     relative to sum |q_i| |c_i| <= |q| |c| of the operands they run on: together below 3 D 2^-24 (1 + 2^-9) for D <= 2^14;
//   * 2^-22 for what the scaling and centring themselves round: c - mu is one fp32 subtraction per component (2^-24
//     relative), a component 2^126 below its row's largest may flush when it is scaled;
// both against norms that dominate either operand: |q'| + |dq| >= |q16| and cmax' + dcmax >= |c16|, |c'| for every row.
// The centred image's term (the canonical chain runs on the UNcentred rows) and the subnormal term are added by the caller.
// Every rounding of the bound's own arithmetic goes upward: the norms arrive rounded up and the sum is multiplied by
// 1 + 2^-18, sixty-four times the 2^-24 a single fp32 operation on positive terms can lose, for fewer than sixteen of them.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ICD_HD __host__ __device__
#else
#define ICD_HD
#endif

namespace icd {

constexpr float CERT_ROUND_UP = 1.0f + 3.814697265625e-6f;   // 1 + 2^-18

// relative weight of the summation and scaling terms (times (|q'| + |dq|) (cmax' + dcmax))
ICD_HD inline float cert_acc_rel(int dim) {
    return (3.0f * (float)dim * 5.9604645e-8f * (1.0f + 1.953125e-3f) + 2.384185791015625e-7f) * CERT_ROUND_UP;
}

// an upper bound of |c16| and |c'| of every corpus row
ICD_HD inline float cert_cmax16(float cmax, float dcmax) { return (cmax + dcmax) * CERT_ROUND_UP; }

// the rounding and summation part of eps for one query: qn = |q'|, qres = |dq| (both rounded up)
ICD_HD inline float cert_eps_round(float qn, float qres, float cmax16, float dcmax, float acc_rel) {
    return (qres * cmax16 + qn * dcmax + acc_rel * ((qn + qres) * cmax16)) * CERT_ROUND_UP;
}

}  // namespace icd
