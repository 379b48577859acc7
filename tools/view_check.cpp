// Stand-alone host check of bh_view's defaults and argument validation (csrc/render_view.hpp,
// the code bh_default_view and bh_render_bodies run before anything touches the device).
// No GPU and no engine library needed; meant to be built with the sanitizers:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iinclude -Ibarnes-hut-n-body_amd/csrc tools/view_check.cpp -o view_check && ./view_check
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "render_view.hpp"

static int failures = 0;

static void expect(const char *what, bh_view v, bool ok) {
    const char *why = bh::view_error(v);
    if ((why == nullptr) != ok || (why && std::strlen(why) == 0)) {
        std::printf("FAIL %s: %s\n", what, why ? why : "accepted");
        ++failures;
    }
}

int main() {
    bh_view d;
    std::memset(&d, 0xA5, sizeof(d));
    bh::view_defaults(&d);
    if (d.view_x != 0.0 || d.view_y != 0.0 || d.zoom != 1.0 || d.width != 2400 ||
        d.height != 800 || d.heavy_mass != 1000.0) {
        std::printf("FAIL defaults\n");
        ++failures;
    }
    const double inf = std::numeric_limits<double>::infinity();
    const double nan = std::numeric_limits<double>::quiet_NaN();
    bh_view v = d;
    expect("defaults", v, true);
    v = d, v.zoom = 0.0, expect("zoom 0", v, false);
    v = d, v.zoom = -1.0, expect("zoom < 0", v, false);
    v = d, v.zoom = nan, expect("zoom NaN", v, false);
    v = d, v.zoom = inf, expect("zoom inf", v, false);
    v = d, v.zoom = 5e-324, expect("zoom denormal", v, true);
    v = d, v.heavy_mass = nan, expect("heavy_mass NaN", v, false);
    v = d, v.heavy_mass = inf, expect("heavy_mass inf", v, true);
    v = d, v.heavy_mass = -inf, expect("heavy_mass -inf", v, true);
    v = d, v.view_x = nan, v.view_y = inf, expect("origin NaN / inf", v, true);
    v = d, v.width = 0, expect("width 0", v, false);
    v = d, v.width = -1, expect("width -1", v, false);
    v = d, v.width = 16385, expect("width 16385", v, false);
    v = d, v.height = 0, expect("height 0", v, false);
    v = d, v.height = 16385, expect("height 16385", v, false);
    v = d, v.width = std::numeric_limits<int32_t>::max(), v.height = v.width;
    expect("INT_MAX x INT_MAX", v, false);
    v = d, v.width = std::numeric_limits<int32_t>::min(), expect("width INT_MIN", v, false);
    v = d, v.width = 16384, v.height = 1024, expect("16384 x 1024 (1 << 24)", v, true);
    v = d, v.width = 16384, v.height = 1025, expect("16384 x 1025", v, false);
    v = d, v.width = 4096, v.height = 4096, expect("4096 x 4096", v, true);
    v = d, v.width = 4097, v.height = 4096, expect("4097 x 4096", v, false);
    v = d, v.width = 1, v.height = 1, expect("1 x 1", v, true);
    std::printf(failures ? "view_check: %d failures\n" : "view_check: ok\n", failures);
    return failures ? 1 : 0;
}
