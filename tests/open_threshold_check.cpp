// Host check of csrc/open_threshold.hpp (compiled and run by tests/test_open_threshold.py with
// -ffp-contract=off): for every case the reference's criterion on the node's own s2,
//     S_d < RN(theta2 * d2),  S_d = s2_0 * 2^-k,  k = 2 x depth,
// must equal the walk's threshold form d2 >= ldexp(thr0, -k).  Prints the case count; exit
// status 1 with the first disagreements on stderr otherwise.
#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "open_threshold.hpp"

namespace {

uint64_t rng_state = 0x243F6A8885A308D3ull;
uint64_t next_u64() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
double unit() { return (double)(next_u64() >> 11) * 0x1p-53; }  // [0, 1)

double from_bits(uint64_t b) {
    double d;
    std::memcpy(&d, &b, sizeof d);
    return d;
}
uint64_t to_bits(double d) {
    uint64_t b;
    std::memcpy(&b, &d, sizeof b);
    return b;
}

long long cases = 0, failures = 0;

void fail(const char *what, double s2_0, double theta2, double thr0, int k, double d2) {
    if (++failures <= 10)
        std::fprintf(stderr, "%s: s2_0=%a theta2=%a thr0=%a k=%d d2=%a\n", what, s2_0, theta2, thr0,
                     k, d2);
}

// one (root, theta) pair: minimality of thr0, then every depth with d2 around the scaled
// threshold and across the fast path's range
void check_pair(double s2_0, double theta, int random_per_depth) {
    const double theta2 = theta * theta;
    const double thr0 = bh::open_threshold(s2_0, theta2);
    if (!bh::open_threshold_ok(thr0, theta2)) {
        fail("precondition refused an in-range pair", s2_0, theta2, thr0, 0, 0.0);
        return;
    }
    // the least double with P: P(thr0) and not P(the double below)
    if (!bh::open_p(s2_0, theta2, thr0)) fail("P(thr0) is false", s2_0, theta2, thr0, 0, thr0);
    if (bh::open_p(s2_0, theta2, std::nextafter(thr0, 0.0)))
        fail("P holds below thr0", s2_0, theta2, thr0, 0, std::nextafter(thr0, 0.0));
    for (int k = 0; k <= 254; k += 2) {
        const double S_d = std::ldexp(s2_0, -k);   // exact: s2_0 >= 2^-760
        const double thr = std::ldexp(thr0, -k);   // exact: thr0 >= 2^-760
        // the device's form of the same threshold: k subtracted from the exponent field
        if (to_bits(thr) != to_bits(thr0) - ((uint64_t)k << 52))
            fail("exponent-field threshold differs from ldexp", s2_0, theta2, thr0, k, thr);
        auto one = [&](double d2) {
            if (!(d2 >= 0x1p-600 && d2 <= 0x1p67)) return;  // the fast path's dist2 range
            ++cases;
            const bool reference = S_d < theta2 * d2;  // BHA:226-228
            const bool threshold = d2 >= thr;
            if (reference != threshold) fail("criterion forms disagree", s2_0, theta2, thr0, k, d2);
        };
        for (int u = -4; u <= 4; ++u) one(from_bits(to_bits(thr) + (uint64_t)(int64_t)u));
        for (int j = 0; j < random_per_depth; ++j) {
            // across [2^-600, 2^67], and within a factor 4 of the threshold
            one(std::ldexp(1.0 + unit(), (int)(next_u64() % 667) - 600));
            one(thr * (0.25 + 3.75 * unit()));
        }
    }
}

}  // namespace

int main() {
    // root cells: s2_0 = (2 h_0)^2 with h_0 = max(W, H) / 2 + 2 for several screens, and others
    const double roots[] = {2404.0 * 2404.0, 1004.0 * 1004.0, 1924.0 * 1924.0, 644.0 * 644.0,
                            7.0 * 7.0,       1.0,             0x1p-700,        0x1p900,
                            3.0e9,           1.2345678901234567e-5};
    const double thetas[] = {0.3, 0.5, 0.75, 1.0, 1.6};
    for (double s2_0 : roots)
        for (double th : thetas) check_pair(s2_0, th, 40);
    for (int i = 0; i < 160; ++i) {  // random theta in [2^-8, 2^4), random roots
        const double th = std::ldexp(1.0 + unit(), (int)(next_u64() % 12) - 8);
        const double s2_0 = i % 4 == 0 ? roots[(i / 4) % 10]
                                       : std::ldexp(1.0 + unit(), (int)(next_u64() % 120) - 40);
        check_pair(s2_0, th, 30);
    }
    // the precondition: theta = 1e-200 (theta2 underflows to 0) and 1e200 (overflows) are refused,
    // and so is a theta2 outside [2^-400, 2^400] or a thr0 outside [2^-760, 2^1000]
    const double s2 = 2404.0 * 2404.0;
    for (double th : {1e-200, 1e200, 1e-100, 1e100, 0.0}) {
        const double t2 = th * th;
        ++cases;
        if (bh::open_threshold_ok(bh::open_threshold(s2, t2), t2))
            fail("precondition accepted an out-of-range theta", s2, t2, bh::open_threshold(s2, t2), 0, th);
    }
    ++cases;
    if (bh::open_threshold_ok(bh::open_threshold(0x1p-900, 0.25), 0.25))
        fail("precondition accepted thr0 below 2^-760", 0x1p-900, 0.25, 0.0, 0, 0.0);
    ++cases;
    if (bh::open_threshold_ok(bh::open_threshold(0x1p990, 0x1p-20), 0x1p-20))
        fail("precondition accepted thr0 above 2^1000", 0x1p990, 0x1p-20, 0.0, 0, 0.0);
    ++cases;
    if (bh::open_threshold_ok(bh::open_threshold(std::nan(""), 0.25), 0.25) ||
        bh::open_threshold_ok(bh::open_threshold(INFINITY, 0.25), 0.25))
        fail("precondition accepted a non-finite s2_0", 0.0, 0.25, 0.0, 0, 0.0);
    std::printf("cases %lld failures %lld\n", cases, failures);
    return failures ? 1 : 0;
}
