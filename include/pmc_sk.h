/*
 * pmc_sk.h -- numerical definition of the collective density modes rho(k) = sum_j exp(i k.r_j)
 * behind the static structure factor S(k), shared by the HIP kernel (k_sk), the host API
 * (pmc_density_modes) and the plain-C restatement the tests use (tests/sk_ref.c).  Like
 * pmc_probe.h it is C99 and HIP C++, built with contraction off.  The wave vectors are the box's
 * reciprocal lattice, k = 2 pi (h_x / L_x, h_y / L_y, h_z / L_z) with integer h, so rho(k) is periodic
 * by construction; with an integer phase it is defined bit for bit: every output is an integer sum,
 * exact in any order, independent of the launch shape and exactly additive over slab contexts.
 * S(k) = |rho(k)|^2 / N is taken on the host in float64 (pmc_amd.observables.structure_factor).
 *
 * Limits: PMC_SK_MAX_K vectors per call, every |h_d| <= PMC_SK_MAX_H.
 *
 * Position word.  Per axis d with L_d = (float)cps_d * w (cps_z the GLOBAL count: coordinates are
 * global, as everywhere) the host computes scale_d = pmc_sk_scale(L_d) = 2^32 / L_d, one float
 * division, and
 *     q_d = pmc_sk_word(x_d, scale_d) = (uint32_t)(int64_t)floorf(x_d * scale_d):
 * one float multiply, floorf, then the conversion through int64, so that negative values and
 * x = +L/2 wrap modulo 2^32 instead of overflowing.  A particle a few ulp outside (-L/2, L/2]
 * ("Cell bounds") wraps like any other.  No image shifts and no halo cells are involved.
 *
 * Phase of vector m = (h_x, h_y, h_z), each cast to uint32:
 *     p = h_x * q_x + h_y * q_y + h_z * q_z   in uint32 arithmetic, wrapping:
 * the exact phase of the quantised position in units of 2^-32 turns.
 *
 * Term (pmc_sk_term).  u = (float)(p >> 8) * 2^-24 is exact, lies in [0, 1) and 4u is exact, as
 * pmc_det_sincos_2pi requires; (s, c) = pmc_det_sincos_2pi(u); particle j adds pmc_to_fixed_f32(c) to
 * re[m] and pmc_to_fixed_f32(s) to im[m], int64 sums in 2^-32 units.  |sum| <= N * 2^32: no wrap for
 * N < 2^31.  pmc_sk_fixed_unit is pmc_to_fixed_f32 without the branches |f| <= 1 cannot take, the
 * same bits (tests/test_sk_ref.py checks every term of the 2^24 phases).
 *
 * Which particles: every occupied slot of every OWNED cell, the counts clamped to [0, nmax] as the
 * other observables read them; halo planes are never read.
 *
 * Outputs: pmc_sk_obs (pmc.h: particles), int64 re[nk], int64 im[nk].  The zero vector gives
 * re = particles << 32 and im = 0 exactly (u = 0 yields s = +0, c = 1).
 *
 * Error budget: one term differs from cos / sin of the exact word phase
 * 2 pi p / 2^32 by less than 4.8e-7 (pmc_det_sincos_2pi 9.76e-8 over all 2^24 inputs, the dropped 8
 * bits 2 pi 255 / 2^32 = 3.73e-7, the fixed-point rounding 2^-33); against the true float position
 * the word adds less than 2^-24 turn per unit of |h_d|, i.e. 2 pi sum_d |h_d| 2^-24 per particle.
 */
#ifndef PMC_SK_H
#define PMC_SK_H

#include "pmc_detmath.h"

#define PMC_SK_MAX_K 4096
#define PMC_SK_MAX_H 1024

/* host: 2^32 / L, one float division */
static inline float pmc_sk_scale(float L) { return 4294967296.0f / L; }

/* position word: the coordinate in units of 2^-32 box lengths, modulo 2^32 */
PMC_HD uint32_t pmc_sk_word(float x, float scale) {
    return (uint32_t)(int64_t)__builtin_floorf(x * scale);
}

/* phase of (hx, hy, hz) at the words (qx, qy, qz), in 2^-32 turns */
PMC_HD uint32_t pmc_sk_phase(int32_t hx, int32_t hy, int32_t hz, uint32_t qx, uint32_t qy, uint32_t qz) {
    return (uint32_t)hx * qx + (uint32_t)hy * qy + (uint32_t)hz * qz;
}

/* pmc_to_fixed_f32(f) for |f| <= 1 (exponent <= 127: the left shift is at most 9 and nothing
 * clamps), bit for bit */
PMC_HD int64_t pmc_sk_fixed_unit(float f) {
    const uint32_t b = pmc_fbits(f);
    const uint32_t ex = (b >> 23) & 0xFFu;
    const uint32_t m = (b & 0x7FFFFFu) | 0x800000u;
    const int sh = (int)ex - 118;
    const int sl = sh < 0 ? 0 : sh;
    const int sr = sh >= 0 ? 1 : (-sh > 25 ? 25 : -sh);
    const uint64_t left = (uint64_t)m << sl;
    const uint64_t right = (uint64_t)((m + (1u << (sr - 1))) >> sr);
    const uint64_t q = sh >= 0 ? left : right;
    return (b >> 31) ? -(int64_t)q : (int64_t)q;
}

/* what one particle adds to re / im of a vector with phase p: the definition */
PMC_HD void pmc_sk_term(uint32_t p, int64_t* re_add, int64_t* im_add) {
    const float u = (float)(p >> 8) * 0x1p-24f;
    float s, c;
    pmc_det_sincos_2pi(u, &s, &c);
    *re_add = pmc_to_fixed_f32(c);
    *im_add = pmc_to_fixed_f32(s);
}

/* the same through pmc_sk_fixed_unit (|s|, |c| <= 1): the kernel's form */
PMC_HD void pmc_sk_term_unit(uint32_t p, int64_t* re_add, int64_t* im_add) {
    const float u = (float)(p >> 8) * 0x1p-24f;
    float s, c;
    pmc_det_sincos_2pi(u, &s, &c);
    *re_add = pmc_sk_fixed_unit(c);
    *im_add = pmc_sk_fixed_unit(s);
}

#endif /* PMC_SK_H */
