// C++ host mirror of the reference's Kotlin surface (BarnesHutAlg.kt = BHA, Config.kt = CFG)
// over the C-ABI in include/bh_engine.h.  Same names, same argument meaning, same call
// pattern as NBodyPanel uses (PNL:103,144,224-233,262,285,291,302,333-340): a caller that
// drove the Kotlin PhysicsEngine drives this one unchanged.
//
// Error behaviour: the reference has no error channel (impossible states are NPEs); here a
// device or argument error throws std::runtime_error carrying bh_last_error().
#pragma once
#include <functional>
#include <stdexcept>
#include <vector>

#include "bh_engine.h"

namespace bh {

// BHA:21-25
struct Body {
    double x, y, vx, vy, m;
};

// BHA:53-82
struct Quad {
    double cx, cy, h;
    bool contains(const Body &b) const {  // BHA:61-62
        return b.x >= cx - h && b.x < cx + h && b.y >= cy - h && b.y < cy + h;
    }
    Quad child(int which) const;  // BHA:73-81
};

// CFG:2-39 — the mutable global the engine reads live at every step().
struct Config {
    static inline int WIDTH_PX = 2400;    // CFG:5
    static inline int HEIGHT_PX = 800;    // CFG:8
    static inline double G = 80.0;        // CFG:11
    static inline double DT = 0.005;      // CFG:14
    static inline double SOFTENING = 1.0; // CFG:17
    static inline const double SOFT2 = 1.0 * 1.0;  // CFG:20 (a val: frozen at init)
    static inline double theta = 0.30;    // CFG:23
    static inline double R = 100.0;       // CFG:26
    static inline int N = 5000;           // CFG:29
    static constexpr double CENTRAL_MASS = 50000.0;          // CFG:32
    static constexpr double MIN_R = 8.0;                     // CFG:35
    static constexpr double TOTAL_SATELLITE_MASS = 5000.0;   // CFG:38
};

// The debug view returned by getTreeForDebug() (BHA:329): visitQuads (BHA:265-274).
class BHTree {
public:
    explicit BHTree(std::vector<Quad> quads) : quads_(std::move(quads)) {}
    void visitQuads(const std::function<void(const Quad &)> &visit) const {
        for (const Quad &q : quads_) visit(q);
    }
    size_t size() const { return quads_.size(); }

private:
    std::vector<Quad> quads_;  // pre-order, as the recursive visit produces them
};

// BHA:287-533
class PhysicsEngine {
public:
    // PhysicsEngine(initialBodies) — adopts the caller's list (BHA:295) on HIP device `device`.
    explicit PhysicsEngine(std::vector<Body> &initialBodies, int device = 0);
    // ... over several GPUs behind one handle (bh_create_multi_list; repeats allowed)
    PhysicsEngine(std::vector<Body> &initialBodies, const std::vector<int> &devices);
    ~PhysicsEngine();
    PhysicsEngine(const PhysicsEngine &) = delete;
    PhysicsEngine &operator=(const PhysicsEngine &) = delete;

    void step();                                      // BHA:405-439
    const std::vector<Body> &getBodies() const;       // BHA:335
    void resetBodies(std::vector<Body> &newBodies);   // BHA:342-349
    BHTree getTreeForDebug();                         // BHA:329-332
    // The panel's overlay of that tree (PNL:326-344) as line-draw counts per pixel, rasterised
    // on the device (bh_render_quads): lines is resized to height x width, row-major; returns the
    // number of cells.  As getTreeForDebug, a fresh tree's jitter is written back into the list.
    int64_t renderTree(const bh_view &view, std::vector<uint32_t> &lines);
    // Conservation read-out of the caller's list (bh_compute_diagnostics; no reference
    // counterpart).  potential = true builds a tree as step()'s first half does -- its jitter is
    // written back into the list -- and adds the potential energy; false only reads the state.
    bh_diagnostics diagnostics(bool potential = true);
    // The field of the caller's list at probe points that are not bodies of it (bh_compute_field;
    // no reference counterpart): ax, ay = F / pm and phi are resized to px.size(), probe order.
    // pm empty: every probe has mass 1.0 (the field per unit mass).  Builds a tree as step()'s
    // first half does -- its jitter is written back into the list; the probes never enter it.
    void computeField(const std::vector<double> &px, const std::vector<double> &py,
                      const std::vector<double> &pm, std::vector<double> &ax,
                      std::vector<double> &ay, std::vector<double> &phi);
    // The same with no cell ever accepted, whatever Config::theta is (bh_compute_field_direct):
    // the exact field of the list, bit-identical to computeField at theta = 0.
    void computeFieldDirect(const std::vector<double> &px, const std::vector<double> &py,
                            const std::vector<double> &pm, std::vector<double> &ax,
                            std::vector<double> &ay, std::vector<double> &phi);
    // The field on a regular grid made on the device (bh_compute_field_grid; bh_field_grid_of_view
    // gives the grid under a view): ax, ay, phi are resized to ny * nx, row-major, each value what
    // computeField returns for that point with pm empty; the device-made summary is returned.
    // planes = false: the summary alone, the vectors are emptied.  Builds a tree as computeField.
    bh_field_grid_stats computeFieldGrid(const bh_field_grid &grid, std::vector<double> &ax,
                                         std::vector<double> &ay, std::vector<double> &phi,
                                         bool planes = true);
    // The tree's force accuracy on the bodies idx[j] of the list (bh_compute_force_error): their
    // accelerations at Config::theta and their exact ones from one build, each resized to
    // idx.size(), and the summary of |a_tree - a_exact| / |a_exact|.  State semantics of step()'s
    // first half -- the jitter is written back into the list.
    bh_force_error forceError(const std::vector<int64_t> &idx, std::vector<double> &axTree,
                              std::vector<double> &ayTree, std::vector<double> &axExact,
                              std::vector<double> &ayExact);

    // The body of the caller's list nearest to (x, y) within r -- the body under the cursor
    // (PNL:133-178 adds bodies by mouse) -- or nullptr (bh_find_neighbors with one probe; no
    // reference counterpart): among the bodies in the tree of non-zero mass, found iff
    // dx*dx + dy*dy <= r*r, ties to the lower list index.  Builds a tree as step()'s first half
    // does -- its jitter is written back into the list; the pointer is into that list.
    Body *pick(double x, double y, double r);

    // The up to k bodies of the caller's list nearest to (x, y) and no farther than rMax, nearest
    // first, ties to the lower list index (bh_find_knn with one probe; no reference counterpart):
    // among the bodies in the tree of non-zero mass; k in 1..64, rMax = +inf for no cap.  Builds
    // a tree as step()'s first half does -- its jitter is written back into the list; the
    // pointers are into that list.
    std::vector<Body *> nearest(double x, double y, int32_t k, double rMax);

    // The friends-of-friends groups of the caller's list at linking length `link`
    // (bh_find_groups; no reference counterpart): one list of bodies per group of at least
    // minMembers members, in catalogue order (ascending lowest list index; within a group
    // ascending list index).  Bodies outside the root cell or of mass 0 are in no group.  Builds
    // a tree as step()'s first half does -- its jitter is written back into the list; the
    // pointers are into that list.
    std::vector<std::vector<Body *>> groups(double link, int64_t minMembers = 2);

    // The radial profile of the caller's list about (x, y) in the frame moving with (vx, vy)
    // (bh_compute_radial_profile; no reference counterpart): bins is resized to edges.size() - 1
    // records, bin k holding the bodies with edges[k] <= R < edges[k + 1]; the summary is
    // returned.  bodies (nullable): pointers into the caller's list that select the population --
    // one list of groups(), for instance -- else every body.  Only reads the state: nothing is
    // written back into the list.
    bh_radial_summary profile(double x, double y, const std::vector<double> &edges,
                              std::vector<bh_radial_bin> &bins, double vx = 0.0, double vy = 0.0,
                              const std::vector<Body *> *bodies = nullptr);

    // Tracers (bh_set_tracers; no reference counterpart): massless test particles of mass 1.0 that
    // every step() carries along on the bodies' own trees and that exert nothing.  A list of the
    // engine's own, kept across resetBodies; vx, vy empty: zeros; empty x, y: no tracers.
    void setTracers(const std::vector<double> &x, const std::vector<double> &y,
                    const std::vector<double> &vx, const std::vector<double> &vy);
    int64_t numTracers() const;
    void getTracers(std::vector<double> &x, std::vector<double> &y, std::vector<double> &vx,
                    std::vector<double> &vy);
    // Their pass of a frame (bh_render_tracers): owner and counts resized to height x width.
    void renderTracers(const bh_view &view, std::vector<uint32_t> &owner,
                       std::vector<uint32_t> &counts);

    double mergeMaxMass = 4000.0;        // BHA:315
    double mergeMinDist = Config::MIN_R; // BHA:321

    bh_engine *handle() { return eng_; }

private:
    void init();
    void pushParams();
    void pushBodies();
    void mapMirror();
    bool bodiesChanged() const;
    void pullBodies(bool afterStep);
    void check(int rc) const;

    std::vector<Body> *bodies_;
    bh_engine *eng_ = nullptr;
    // What the engine holds, in the caller's order: its pinned mirror (two buffers,
    // bh_set_mirror(e, 2)), mapped after every call that changed it.  step() compares the list
    // against it in place while the step already runs (the step writes the other buffer) and
    // re-uploads only when the caller edited a body, so the engine keeps its Morton-ordered state.
    const double *mir_[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    int64_t mirN_ = -1;
};

}  // namespace bh
