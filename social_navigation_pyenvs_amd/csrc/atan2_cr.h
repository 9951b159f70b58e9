// atan2_cr.h -- atan2 in double, correctly rounded (up to the table maker's dilemma at ~2^-100): double-double arithmetic on
// error-free transforms.  Used where the LAST BIT of atan2 decides a result: Moussaid's pair force multiplies a lateral term by
// sign(theta_ij), theta_ij = wrap(atan2(n) - atan2(i) + pi), and with nobody moving theta_ij is the rounding of the two atan2 values
// (+-1e-16).  The reference's atan2 (numpy -> the C library's, the IBM accurate routine) returns the correctly rounded value; so does
// this one, and the sign comes out the same.  The device library's atan2 is within an ulp or two and flips that coin.
//
// atan2(y, x): z = min(|y|, |x|) / max(|y|, |x|) in double-double; c = rint(16 z) / 16; t = (z - c) / (1 + z c), |t| <= 1 / 32;
// atan z = atan c (table, double-double) + t (1 - t^2 / 3 + ... - t^22 / 23) (Horner in double-double); the octant and quadrant folded
// with pi / 2 and pi in double-double; the result is the rounded sum.  Zeros, infinities, NaN and ratios below 2^-60: the library's atan2
// (nothing to decide there).  Compile with contraction OFF: the error-free transforms below rely on every operation being rounded as written.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define CR_HD __host__ __device__ inline
#else
#define CR_HD inline
#endif

namespace crmath {

struct DD { double hi, lo; };

CR_HD DD two_sum(double a, double b) { const double s = a + b, bb = s - a; return DD{s, (a - (s - bb)) + (b - bb)}; }
CR_HD DD fast_two_sum(double a, double b) { const double s = a + b; return DD{s, b - (s - a)}; }   // |a| >= |b|
CR_HD DD two_prod(double a, double b) { const double p = a * b; return DD{p, fma(a, b, -p)}; }
CR_HD DD dd_add(DD a, DD b)
{
    DD s = two_sum(a.hi, b.hi);
    const DD t = two_sum(a.lo, b.lo);
    s = fast_two_sum(s.hi, s.lo + t.hi);
    return fast_two_sum(s.hi, s.lo + t.lo);
}
CR_HD DD dd_neg(DD a) { return DD{-a.hi, -a.lo}; }
CR_HD DD dd_mul(DD a, DD b)
{
    DD p = two_prod(a.hi, b.hi);
    p.lo += a.hi * b.lo + a.lo * b.hi;
    return fast_two_sum(p.hi, p.lo);
}
CR_HD DD dd_mul_d(DD a, double b)
{
    DD p = two_prod(a.hi, b);
    p.lo += a.lo * b;
    return fast_two_sum(p.hi, p.lo);
}
CR_HD DD dd_div(DD n, DD d)
{
    const double q1 = n.hi / d.hi;
    const DD r = dd_add(n, dd_neg(dd_mul_d(d, q1)));
    const double q2 = r.hi / d.hi;
    const DD r2 = dd_add(r, dd_neg(dd_mul_d(d, q2)));
    const double q3 = r2.hi / d.hi;
    const DD q = fast_two_sum(q1, q2);
    return dd_add(q, DD{q3, 0.0});
}

CR_HD double atan2_cr(double y, double x)
{
    constexpr DD kAtanTab[17] = {{0x0.0p+0, 0x0.0p+0}, {0x1.ff55bb72cfdeap-5, -0x1.c934d86d23f1dp-60}, {0x1.fd5ba9aac2f6ep-4, -0x1.cd37686760c17p-59}, {0x1.7b97b4bce5b02p-3, 0x1.347b0b4f881cap-58}, {0x1.f5b75f92c80ddp-3, 0x1.8ab6e3cf7afbdp-57}, {0x1.362773707ebccp-2, -0x1.963a544b672d8p-57}, {0x1.6f61941e4def1p-2, -0x1.c63aae6f6e918p-56}, {0x1.a64eec3cc23fdp-2, -0x1.24dec1b50b7ffp-56}, {0x1.dac670561bb4fp-2, 0x1.a2b7f222f65e2p-56}, {0x1.0657e94db30d0p-1, -0x1.d5b495f6349e6p-56}, {0x1.1e00babdefeb4p-1, -0x1.928df287a668fp-58}, {0x1.345f01cce37bbp-1, 0x1.1021137c71102p-55}, {0x1.4978fa3269ee1p-1, 0x1.2419a87f2a458p-56}, {0x1.5d58987169b18p-1, 0x1.0028e4bc5e7cap-57}, {0x1.700a7c5784634p-1, -0x1.8c34d25aadef6p-56}, {0x1.819d0b7158a4dp-1, -0x1.bf76229d3b917p-56}, {0x1.921fb54442d18p-1, 0x1.1a62633145c07p-55}};
    constexpr DD kOdd[11] = {{-0x1.5555555555555p-2, -0x1.5555555555555p-56}, {0x1.999999999999ap-3, -0x1.999999999999ap-57}, {-0x1.2492492492492p-3, -0x1.2492492492492p-57}, {0x1.c71c71c71c71cp-4, 0x1.c71c71c71c71cp-58}, {-0x1.745d1745d1746p-4, 0x1.745d1745d1746p-59}, {0x1.3b13b13b13b14p-4, -0x1.3b13b13b13b14p-58}, {-0x1.1111111111111p-4, -0x1.1111111111111p-60}, {0x1.e1e1e1e1e1e1ep-5, 0x1.e1e1e1e1e1e1ep-61}, {-0x1.af286bca1af28p-5, -0x1.af286bca1af28p-59}, {0x1.8618618618618p-5, 0x1.8618618618618p-59}, {-0x1.642c8590b2164p-5, -0x1.642c8590b2164p-60}};
    constexpr DD kPi = {0x1.921fb54442d18p+1, 0x1.1a62633145c07p-53}, kHalfPi = {0x1.921fb54442d18p+0, 0x1.1a62633145c07p-54};
    const double ay = fabs(y), ax = fabs(x);
    const bool swap = ay > ax;
    const double num = swap ? ax : ay, den = swap ? ay : ax;
    // nothing for the last bit to decide (and no double-double range to work in): the library's value
    if (!(num > 0.0) || !(den < 1e300) || !(num > 1e-290) || num < den * 0x1p-60) return atan2(y, x);
    const DD z = dd_div(DD{num, 0.0}, DD{den, 0.0});
    const double kf = rint(z.hi * 16.0);
    const int k = (int)kf;
    const double c = kf * 0.0625;
    const DD dz = dd_add(z, DD{-c, 0.0});
    const DD dn = dd_add(DD{1.0, 0.0}, dd_mul_d(z, c));
    const DD t = dd_div(dz, dn);
    const DD w = dd_mul(t, t);
    DD s = kOdd[10];
#pragma unroll
    for (int j = 9; j >= 0; --j) s = dd_add(dd_mul(s, w), kOdd[j]);
    s = dd_add(dd_mul(s, w), DD{1.0, 0.0});
    DD r = dd_add(kAtanTab[k], dd_mul(t, s));
    if (swap) r = dd_add(kHalfPi, dd_neg(r));
    if (x < 0.0) r = dd_add(kPi, dd_neg(r));
    const double a = r.hi + r.lo;
    return y < 0.0 ? -a : a;
}

} // namespace crmath
