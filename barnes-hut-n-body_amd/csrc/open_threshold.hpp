// The opening criterion as one threshold on dist2 (host and device; plain C++, no HIP needed).
//
// The reference accepts an internal node of depth d iff s2_d < RN(theta2 * dist2) (BHA:226-228)
// with s2_d = s2_0 * 2^-k exactly, k = 2d <= 255.  Let P(t) := s2_0 < RN(theta2 * t).  The product
// by theta2 > 0 and the rounding are monotone, so there is a least double thr0 with P(t) true for
// every t >= thr0 and false below it.  A scaling by 2^k commutes with the rounding while nothing
// leaves the normal range, hence
//     s2_d < RN(theta2 * dist2)  <=>  s2_0 < RN(theta2 * (2^k dist2))  <=>  2^k dist2 >= thr0
//                                <=>  dist2 >= thr0 * 2^-k,
// the last step exact while thr0 * 2^-k is normal: the walk compares dist2 with a threshold whose
// exponent field is thr0's less k -- no product by theta2, and a leaf is the threshold +0.0.
//
// Ranges.  The fast walks have dist2 in [2^-600, 2^67] (fastmath.hpp, lane_fast_ok) and
// s2_0 in [2^-760, 2^1000] (fast_s2_ok).  With theta2 in [2^-400, 2^400]:
//     theta2 * dist2        in [2^-1000, 2^467]   normal and finite,
//     theta2 * 2^k * dist2  in [2^-1000, 2^722]   normal and finite (2^k dist2 <= 2^322 is exact),
//     s2_0 * 2^-k           >= 2^-1015            normal,
// so both scalings above are exact.  thr0 ~ s2_0 / theta2 could still leave the range in which the
// exponent subtraction is exact, so it is bounded by itself: thr0 in [2^-760, 2^1000] keeps
// thr0 * 2^-k normal for every k <= 255.  open_threshold_ok() is that precondition; a launch that
// fails it takes the IEEE walk.
#pragma once
#include <cmath>
#include <cstdint>
#include <limits>

#if defined(__HIPCC__)
#define BH_THR_HD __host__ __device__
#else
#define BH_THR_HD
#endif

namespace bh {

// P(t): the single IEEE product of the device's criterion (build with -ffp-contract=off).
BH_THR_HD inline bool open_p(double s2_0, double theta2, double t) { return s2_0 < theta2 * t; }

// Wave-uniform precondition of the threshold form (beside fast_s2_ok): see the ranges above.
// thr0 = 0.0 (open_threshold's "none") fails it.
BH_THR_HD inline bool open_threshold_ok(double thr0, double theta2) {
    return thr0 >= 0x1p-760 && thr0 <= 0x1p1000 && theta2 >= 0x1p-400 && theta2 <= 0x1p400;
}

// The least double t with P(t), found from s2_0 / theta2 by single steps (the quotient is within
// a few ulp of it); 0.0 if there is none within reach (non-finite or non-positive operands, a
// quotient that overflows or is subnormal) -- open_threshold_ok(0.0, .) is false.
inline double open_threshold(double s2_0, double theta2) {
    if (!(s2_0 > 0.0 && theta2 > 0.0) || !std::isfinite(s2_0) || !std::isfinite(theta2)) return 0.0;
    double t = s2_0 / theta2;
    if (!std::isfinite(t) || !(t >= 0x1p-1020)) return 0.0;
    const double inf = std::numeric_limits<double>::infinity();
    for (int i = 0; i < 64 && !open_p(s2_0, theta2, t); ++i) t = std::nextafter(t, inf);
    if (!std::isfinite(t) || !open_p(s2_0, theta2, t)) return 0.0;
    for (int i = 0; i < 64; ++i) {
        const double lower = std::nextafter(t, 0.0);
        if (!open_p(s2_0, theta2, lower)) return t;
        t = lower;
    }
    return 0.0;
}

}  // namespace bh
