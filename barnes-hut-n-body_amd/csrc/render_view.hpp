// bh_view's defaults and argument check (include/bh_engine.h, bh_render_bodies).  Host code with
// no device dependency, so that it also builds into a stand-alone checker (tools/view_check.cpp).
#pragma once

#include <cmath>
#include <cstdint>

#include "bh_engine.h"

namespace bh {

constexpr int32_t VIEW_MAX_SIDE = 16384;
constexpr int64_t VIEW_MAX_PIXELS = int64_t(1) << 24;

inline void view_defaults(bh_view *v) {
    v->view_x = 0.0;
    v->view_y = 0.0;
    v->zoom = 1.0;
    v->width = 2400;   // CFG:5
    v->height = 800;   // CFG:8
    v->heavy_mass = 1000.0;  // PNL:303
}

// null if the view is usable, else what is wrong with it
inline const char *view_error(const bh_view &v) {
    if (!std::isfinite(v.zoom) || !(v.zoom > 0.0)) return "bh_view: zoom must be finite and > 0";
    if (std::isnan(v.heavy_mass)) return "bh_view: heavy_mass is NaN";
    if (v.width < 1 || v.width > VIEW_MAX_SIDE || v.height < 1 || v.height > VIEW_MAX_SIDE)
        return "bh_view: width and height must be in 1..16384";
    if ((int64_t)v.width * (int64_t)v.height > VIEW_MAX_PIXELS)
        return "bh_view: width * height must not exceed 1 << 24";
    return nullptr;
}

}  // namespace bh
