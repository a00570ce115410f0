// The scene plan (csrc/rt_scene_plan.h) on its own: what rt_scene_create decides before it uploads anything, rule by rule.  Every
// expected value below is written out by hand from the rule the comment names; none is computed by the code under test.
// tests/test_scene_plan_host.py builds this with -fsanitize=address,undefined and runs it; no HIP call, no device.
//
// Boxes are chosen so that every union, area and cost is a small integer: a "bar" is [x0, x1] x [0, 1] x [0, 1], whose surface
// area is 2 (w + 1 + w) = 4 w + 2 for w = x1 - x0; the "huge" box is [-50, 50]^3 with area 6 * 100^2 = 60 000, and the union of
// anything below with it is itself.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "rt_scene_plan.h"

using namespace rt_scene_plan;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static_assert(sizeof(rt_node) == 32, "nodes are compared as 32 bytes");

static rt_node node(float x0, float y0, float z0, float x1, float y1, float z1, int32_t skip, int32_t prim) {
    rt_node n;
    n.bmin[0] = x0; n.bmin[1] = y0; n.bmin[2] = z0; n.skip = skip;
    n.bmax[0] = x1; n.bmax[1] = y1; n.bmax[2] = z1; n.prim = prim;
    return n;
}
static rt_node bar(float x0, float x1, int32_t skip, int32_t prim) { return node(x0, 0, 0, x1, 1, 1, skip, prim); }
static rt_node huge(int32_t skip, int32_t prim) { return node(-50, -50, -50, 50, 50, 50, skip, prim); }
static bool same(const std::vector<rt_node>& got, std::initializer_list<rt_node> want) {
    if (got.size() != want.size()) return false;
    size_t i = 0;
    for (const rt_node& w : want) if (std::memcmp(&got[i++], &w, sizeof(rt_node)) != 0) return false;
    return true;
}
static bool all_kept(const collapse_plan& p, size_t n) {
    if (p.keep.size() != n) return false;
    for (char k : p.keep) if (k != 1) return false;
    return true;
}
static int32_t word(float f) { int32_t w; std::memcpy(&w, &f, 4); return w; }

// ---- "Collapse"

// root (node 0) over two leaves; 100 rays visit the root and pass[0] of them pass its box.  Keeping the root costs
// 100 + 2 pass[0] tests, dropping it 2 * 100: it is kept iff pass[0] <= 50.
static void check_collapse_two_leaves() {
    const rt_node tree[3] = {bar(0, 4, 3, -1), bar(0, 1, 2, 7), bar(3, 4, 3, 8)};
    collapse_plan p;
    // n < 3 is left alone
    CHECK(!plan_collapse(tree + 1, 2, {1.0, 1.0}, 100.0, p) && all_kept(p, 2));
    CHECK(!plan_collapse(tree, 3, {100.0, 0.0, 0.0}, 0.0, p) && all_kept(p, 3));   // no ray visited the root: nothing to decide on

    CHECK(plan_collapse(tree, 3, {100.0, 30.0, 30.0}, 100.0, p));   // a root every ray passes: dropped
    CHECK(p.keep.size() == 3 && p.keep[0] == 0 && p.keep[1] == 1 && p.keep[2] == 1);
    CHECK(p.tests_before == 3.0 && p.tests_after == 2.0);            // (100 + 100 + 100) / 100; (100 + 100) / 100
    CHECK(same(build_walk_array(tree, 3, p.keep), {bar(0, 1, 1, 7), bar(3, 4, 2, 8)}));

    CHECK(plan_collapse(tree, 3, {10.0, 5.0, 5.0}, 100.0, p) && all_kept(p, 3));   // a root few rays pass: kept
    CHECK(p.tests_before == 1.2 && p.tests_after == 1.2);            // (100 + 10 + 10) / 100 either way
    CHECK(same(build_walk_array(tree, 3, p.keep), {tree[0], tree[1], tree[2]}));

    CHECK(plan_collapse(tree, 3, {50.0, 5.0, 5.0}, 100.0, p) && all_kept(p, 3));   // the tie, 200 tests either way: keep <= drop keeps
    CHECK(p.tests_before == 2.0 && p.tests_after == 2.0);
}

// root 0 over (middle 1 over leaves 2, 3) and leaf 4; 100 rays, 20 pass the root and all 20 pass the middle.
//   below the middle: a leaf costs what its nearest kept ancestor passes
//   middle under a kept root: kept 20 + 2 * 20 = 60, dropped 2 * 20 = 40 -> dropped (40)
//   middle under a dropped root: kept 100 + 40 = 140, dropped 200 -> 140
//   root: kept 100 + 40 + 20 (leaf 4) = 160, dropped 140 + 100 = 240 -> kept
// before: 100 + 20 (middle) + 20 + 20 + 20 (the three leaves) = 180
static void check_collapse_middle_dropped() {
    const rt_node tree[5] = {node(0, 0, 0, 10, 10, 10, 5, -1), node(0, 0, 0, 4, 4, 4, 4, -1), node(0, 0, 0, 1, 1, 1, 3, 11), node(2, 2, 2, 3, 3, 3, 4, 12),
                             node(6, 6, 6, 7, 7, 7, 5, 13)};
    collapse_plan p;
    CHECK(plan_collapse(tree, 5, {20.0, 20.0, 1.0, 2.0, 3.0}, 100.0, p));
    CHECK(p.keep.size() == 5 && p.keep[0] == 1 && p.keep[1] == 0 && p.keep[2] == 1 && p.keep[3] == 1 && p.keep[4] == 1);
    CHECK(p.tests_before == 1.8 && p.tests_after == 1.6);
    // the kept nodes in order; a link to node k becomes the number of kept nodes before k: 5 -> 4, 3 -> 2, 4 -> 3
    CHECK(same(build_walk_array(tree, 5, p.keep), {node(0, 0, 0, 10, 10, 10, 4, -1), node(0, 0, 0, 1, 1, 1, 2, 11), node(2, 2, 2, 3, 3, 3, 3, 12),
                                                   node(6, 6, 6, 7, 7, 7, 4, 13)}));
}

// what the argument for dropping a node does not cover is walked as given
static void check_collapse_leaves_alone() {
    collapse_plan p;
    const std::vector<double> every_ray = {100.0, 100.0, 100.0, 100.0};   // (would drop every interior node of a sound tree)
    {   // a child box poking out of its parent's (4.5 > 4)
        const rt_node tree[3] = {bar(0, 4, 3, -1), bar(0, 1, 2, 7), bar(3, 4.5f, 3, 8)};
        CHECK(!plan_collapse(tree, 3, every_ray, 100.0, p) && all_kept(p, 3));
        CHECK(same(build_walk_array(tree, 3, p.keep), {tree[0], tree[1], tree[2]}));
    }
    {   // a dangling child range: the root's range ends at 2, node 2 has no parent
        const rt_node tree[3] = {bar(0, 4, 2, -1), bar(0, 1, 2, 7), bar(3, 4, 3, 8)};
        CHECK(!plan_collapse(tree, 3, every_ray, 100.0, p) && all_kept(p, 3));
    }
    {   // ... an interior node with no child at all
        const rt_node tree[3] = {bar(0, 4, 3, -1), bar(0, 1, 2, -1), bar(3, 4, 3, 8)};
        CHECK(!plan_collapse(tree, 3, every_ray, 100.0, p) && all_kept(p, 3));
    }
    {   // ... a leaf whose link jumps over its sibling
        const rt_node tree[4] = {bar(0, 4, 4, -1), bar(0, 1, 3, 7), bar(1, 2, 3, 8), bar(3, 4, 4, 9)};
        CHECK(!plan_collapse(tree, 4, every_ray, 100.0, p) && all_kept(p, 4));
    }
    // a list-like tree: interior node 2 k (depth k) over leaf 2 k + 1 and interior node 2 k + 2; the last node is a leaf at
    // depth `levels`.  61 levels is deeper than 60 and left alone; 60 is planned.
    for (int levels = 60; levels <= 61; ++levels) {
        const int n = 2 * levels + 1;
        std::vector<rt_node> tree;
        for (int k = 0; k < levels; ++k) { tree.push_back(bar(0, 1, n, -1)); tree.push_back(bar(0, 1, 2 * k + 2, k)); }
        tree.push_back(bar(0, 1, n, levels));
        const bool planned = plan_collapse(tree.data(), n, std::vector<double>((size_t)n, 1.0), 1.0, p);
        CHECK(planned == (levels == 60));
        if (levels == 61) CHECK(all_kept(p, (size_t)n));
    }
    // the surface-area prior: 2 (1 * 2 + 2 * 3 + 1 * 3) = 22; an inverted box counts as empty
    const rt_node boxes[2] = {node(0, 0, 0, 1, 2, 3, 2, -1), node(1, 0, 0, 0, 2, 3, 2, 0)};
    const std::vector<double> area = area_passes(boxes, 2);
    CHECK(area.size() == 2 && area[0] == 22.0 && area[1] == 12.0);   // the second: extents 0, 2, 3 -> 2 * (2 * 3)
}

// ---- "Regroup": the huge leaf first (the ground sphere), then bars A = [0, 1], B = [2, 3], C = [3, 4], D = [5, 6]
static const int32_t GROUND = 40, A = 41, B = 42, C = 43, D = 44;
static std::vector<rt_node> five_leaves() {
    // (any array with these leaves in this order: the interior nodes and the links of the input are not looked at)
    return {huge(6, -1), huge(2, GROUND), bar(0, 1, 3, A), bar(2, 3, 4, B), bar(3, 4, 5, C), bar(5, 6, 6, D)};
}
// {ground, {{A, B}, {C, D}}}
#define PAIRS_TREE {huge(9, -1), huge(2, GROUND), bar(0, 6, 9, -1), bar(0, 3, 6, -1), bar(0, 1, 5, A), bar(2, 3, 6, B), bar(3, 6, 9, -1), bar(3, 4, 8, C), bar(5, 6, 9, D)}
// {ground, {{A, {B, C}}, D}}
#define NEAREST_FIRST_TREE {huge(9, -1), huge(2, GROUND), bar(0, 6, 9, -1), bar(0, 4, 8, -1), bar(0, 1, 5, A), bar(2, 4, 8, -1), bar(2, 3, 7, B), bar(3, 4, 8, C), bar(5, 6, 9, D)}

static void check_regroup() {
    const std::vector<rt_node> in = five_leaves();
    // Top-down.  [ground A B C D]: splitting after the ground costs 60 000 * 1 + area[0, 6] * 4 = 60 000 + 26 * 4; any later split
    // has the ground on the left at 60 000 * 2 or more.  [A B C D]: after A 6 + 18 * 3 = 60, after B 14 * 2 + 14 * 2 = 56, after C
    // 18 * 3 + 6 = 60: after B.
    CHECK(same(regroup_leaves(in.data(), (int)in.size(), 0), PAIRS_TREE));
    // Bottom-up by area.  Neighbour unions: ground+A 60 000, A+B [0, 3] 14, B+C [2, 4] 10, C+D [3, 6] 14: B+C first.  Then A+BC
    // [0, 4] 18 and BC+D [2, 6] 18: the tie goes to the pair further left.  Then ABC+D [0, 6] 26, and the ground last.
    CHECK(same(regroup_leaves(in.data(), (int)in.size(), 1), NEAREST_FIRST_TREE));
    // Bottom-up by sampled rays.  Three rays go up through C alone at x = 3.25, 3.5, 3.75 (from y = -10, z = 0.5, limit 1000); the
    // key is rays + area / (area + 1).  ground+A 3 + 60 000 / 60 001, A+B 0 + 14 / 15, B+C 3 + 10 / 11, C+D 3 + 14 / 15: A+B first,
    // although B+C is the smaller box.  Then AB+C [0, 4] 3 + 18 / 19 against C+D 3 + 14 / 15: the rays tie and the area decides,
    // C+D.  Then AB+CD, and the ground last: the top-down tree, not the area merger's.
    std::vector<float> rays;
    for (float x : {3.25f, 3.5f, 3.75f}) for (float v : {x, -10.0f, 0.5f, 0.0f, 1.0f, 0.0f, 1000.0f}) rays.push_back(v);
    CHECK(same(regroup_leaves(in.data(), (int)in.size(), 2, &rays), PAIRS_TREE));
    // ... rays whose limit ends before the bars (y = 0 is 10 away) see the ground's box only, around their origin: no union but
    // the ground's is seen, and the area decides everything
    std::vector<float> early;
    for (float x : {3.25f, 3.5f, 3.75f}) for (float v : {x, -10.0f, 0.5f, 0.0f, 1.0f, 0.0f, 5.0f}) early.push_back(v);
    CHECK(same(regroup_leaves(in.data(), (int)in.size(), 2, &early), NEAREST_FIRST_TREE));
    // ... and without a sample method 2 is method 1
    const std::vector<float> none;
    CHECK(same(regroup_leaves(in.data(), (int)in.size(), 2, nullptr), NEAREST_FIRST_TREE));
    CHECK(same(regroup_leaves(in.data(), (int)in.size(), 2, &none), NEAREST_FIRST_TREE));

    for (int method = 0; method < 3; ++method) {
        const rt_node interior[2] = {bar(0, 1, 2, -1), bar(0, 1, 2, -1)};
        CHECK(regroup_leaves(interior, 2, method, &rays).empty());                          // zero leaves
        const rt_node one[2] = {bar(0, 4, 2, -1), bar(2, 3, 2, B)};
        CHECK(same(regroup_leaves(one, 2, method, &rays), {bar(2, 3, 1, B)}));              // a single leaf, its link re-pointed
    }
    // Non-finite areas: three slabs unbounded in x at y = [0, 1], [1, 2], [2, 3].  No split has a finite cost, so the top-down
    // splitter takes the middle of [0, 3), 1: {0, {1, 2}}.  Every union has the last key, so the merger takes the leftmost pair:
    // {{0, 1}, 2}.
    const float inf = INFINITY;
    const rt_node slabs[3] = {node(-inf, 0, 0, inf, 1, 1, 1, 50), node(-inf, 1, 0, inf, 2, 1, 2, 51), node(-inf, 2, 0, inf, 3, 1, 3, 52)};
    CHECK(same(regroup_leaves(slabs, 3, 0), {node(-inf, 0, 0, inf, 3, 1, 5, -1), node(-inf, 0, 0, inf, 1, 1, 2, 50), node(-inf, 1, 0, inf, 3, 1, 5, -1),
                                             node(-inf, 1, 0, inf, 2, 1, 4, 51), node(-inf, 2, 0, inf, 3, 1, 5, 52)}));
    // ... the middle, not the first split: of four such slabs, [0, 4) is cut at 2
    const rt_node four[4] = {slabs[0], slabs[1], slabs[2], node(-inf, 3, 0, inf, 4, 1, 4, 53)};
    CHECK(same(regroup_leaves(four, 4, 0), {node(-inf, 0, 0, inf, 4, 1, 7, -1), node(-inf, 0, 0, inf, 2, 1, 4, -1), node(-inf, 0, 0, inf, 1, 1, 3, 50),
                                            node(-inf, 1, 0, inf, 2, 1, 4, 51), node(-inf, 2, 0, inf, 4, 1, 7, -1), node(-inf, 2, 0, inf, 3, 1, 6, 52),
                                            node(-inf, 3, 0, inf, 4, 1, 7, 53)}));
    // Two splits of equal cost: bars [0, 1], [1, 2], [2, 3] cost 6 + 10 * 2 = 26 after the first and 10 * 2 + 6 = 26 after the
    // second; only a strictly smaller cost replaces the best so far, so the first split stays: {0, {1, 2}}.
    const rt_node even[3] = {bar(0, 1, 1, A), bar(1, 2, 2, B), bar(2, 3, 3, C)};
    CHECK(same(regroup_leaves(even, 3, 0), {bar(0, 3, 5, -1), bar(0, 1, 2, A), bar(1, 3, 5, -1), bar(1, 2, 4, B), bar(2, 3, 5, C)}));
    for (int method = 1; method < 3; ++method)
        CHECK(same(regroup_leaves(slabs, 3, method, &rays), {node(-inf, 0, 0, inf, 3, 1, 5, -1), node(-inf, 0, 0, inf, 2, 1, 4, -1), node(-inf, 0, 0, inf, 1, 1, 3, 50),
                                                             node(-inf, 1, 0, inf, 2, 1, 4, 51), node(-inf, 2, 0, inf, 3, 1, 5, 52)}));
}

// ---- the leaves-only array of a scanned scene, the device's link encoding
static void check_scanned_and_encoding() {
    const rt_node tree[3] = {bar(0, 4, 3, -1), bar(0, 1, 2, 7), bar(3, 4, 3, 8)};
    const std::vector<rt_node> untouched = {bar(9, 10, 1, 99)};
    std::vector<rt_node> walk = untouched;
    CHECK(leaves_only_if_scanned(tree, 3, 3, walk));                                        // an array at scan_nodes
    CHECK(same(walk, {bar(0, 1, 1, 7), bar(3, 4, 2, 8)}));
    walk = untouched;
    CHECK(!leaves_only_if_scanned(tree, 3, 2, walk) && same(walk, {bar(9, 10, 1, 99)}));    // one above it: walked, not scanned
    CHECK(!leaves_only_if_scanned(tree, 3, 0, walk) && same(walk, {bar(9, 10, 1, 99)}));    // scanning off
    CHECK(!leaves_only_if_scanned(tree + 1, 2, 24, walk) && same(walk, {bar(9, 10, 1, 99)}));   // all leaves already
    CHECK(!leaves_only_if_scanned(tree, 1, 24, walk) && same(walk, {bar(9, 10, 1, 99)}));   // no leaf at all

    // skip -> ~skip; an interior node's prim -> ~(own index + 1); a leaf's prim stays
    const rt_node nested[5] = {bar(0, 9, 5, -1), bar(0, 4, 4, -1), bar(0, 1, 3, 11), bar(2, 3, 4, 12), bar(6, 7, 5, 13)};
    CHECK(same(device_nodes(nested, 5), {bar(0, 9, -6, -2), bar(0, 4, -5, -3), bar(0, 1, -4, 11), bar(2, 3, -5, 12), bar(6, 7, -6, 13)}));
    CHECK(device_nodes(nullptr, 0).empty());
}

// ---- tier data
// a description of `m` leaves and nothing else: leaf q is the bar [q, q + 1] and holds prim(q)
struct leaf_scene {
    std::vector<rt_node> nodes;
    std::vector<rt_instance> instances;
    std::vector<rt_box> boxes;
    rt_scene_desc d;
    template <class Prim> leaf_scene(int m, Prim prim) {
        for (int q = 0; q < m; ++q) nodes.push_back(bar((float)q, (float)(q + 1), q + 1, prim(q)));
        std::memset(&d, 0, sizeof(d));
        d.nodes = nodes.data(); d.n_nodes = m;
    }
};
static int32_t sphere_q(int q) { return RT_PRIM_REF(RT_PRIM_SPHERE, q); }
static tier_data tiers_of(const leaf_scene& s) { return plan_tier_data(&s.d); }
static bool no_tier_data(const tier_data& t) {
    return !t.present && t.lo.empty() && t.hi.empty() && t.ranges.empty() && t.n_leaves == 0 && t.n_slots == 0 && t.n_media_leaves == 0 &&
           t.media_ord[0] == 0x7FFFFFFF && t.media_ord[1] == 0x7FFFFFFF;
}
static bool same_floats(const float* got, std::initializer_list<float> want) {
    for (float w : want) if (std::memcmp(got++, &w, 4) != 0) return false;
    return true;
}
static void check_tier_data() {
    CHECK(no_tier_data(tiers_of(leaf_scene(0, sphere_q))));
    {   // 65 leaves: two slots of 64, the second holding one leaf and 63 paddings
        const leaf_scene s(65, sphere_q);
        const tier_data t = plan_tier_data(&s.d);
        CHECK(t.present && t.n_leaves == 65 && t.n_slots == 2 && t.n_media_leaves == 0 && t.media_ord[0] == 0x7FFFFFFF && t.media_ord[1] == 0x7FFFFFFF);
        CHECK(t.lo.size() == 512 && t.hi.size() == 512 && t.ranges.size() == 16);
        if (t.lo.size() == 512 && t.hi.size() == 512 && t.ranges.size() == 16) {
            CHECK(same_floats(&t.lo[0], {0, 0, 0}) && word(t.lo[3]) == 0 && same_floats(&t.hi[0], {1, 1, 1}) && word(t.hi[3]) == 0);
            CHECK(same_floats(&t.lo[4 * 63], {63, 0, 0}) && word(t.lo[4 * 63 + 3]) == 63 && same_floats(&t.hi[4 * 63], {64, 1, 1}));
            CHECK(same_floats(&t.lo[4 * 64], {64, 0, 0}) && word(t.lo[4 * 64 + 3]) == 64 && same_floats(&t.hi[4 * 64], {65, 1, 1}) && word(t.hi[4 * 64 + 3]) == 0);
            for (int q = 65; q < 128; ++q)   // the padding: prim -1, a zero box, no instance
                CHECK(same_floats(&t.lo[4 * q], {0, 0, 0}) && word(t.lo[4 * q + 3]) == -1 && same_floats(&t.hi[4 * q], {0, 0, 0}) && word(t.hi[4 * q + 3]) == 0);
            // per slot: the union of its leaves' boxes (the padding is not part of it), two unused floats
            CHECK(same_floats(&t.ranges[0], {0, 0, 0, 64, 1, 1, 0, 0, 64, 0, 0, 65, 1, 1, 0, 0}));
        }
    }
    {   // 64 slots is the most: one lane tests one slot's union
        const tier_data most = tiers_of(leaf_scene(4096, sphere_q));
        CHECK(most.present && most.n_leaves == 4096 && most.n_slots == 64 && most.lo.size() == 16384 && most.ranges.size() == 512);
        CHECK(no_tier_data(tiers_of(leaf_scene(4097, sphere_q))));
    }
    {   // media: the leaf ordinals of at most two; a medium's leaf stays a medium
        auto medium_at = [](int first, int second, int third) {
            return [=](int q) { return q == first ? RT_PRIM_REF(RT_PRIM_MEDIUM, 0) : q == second ? RT_PRIM_REF(RT_PRIM_MEDIUM, 1) : q == third ? RT_PRIM_REF(RT_PRIM_MEDIUM, 2) : sphere_q(q); };
        };
        const tier_data two = tiers_of(leaf_scene(5, medium_at(1, 3, -1)));
        CHECK(two.present && two.n_leaves == 5 && two.n_slots == 1 && two.n_media_leaves == 2 && two.media_ord[0] == 1 && two.media_ord[1] == 3);
        CHECK(two.lo.size() == 256 && word(two.lo[4 * 1 + 3]) == 0x40000000 && word(two.lo[4 * 3 + 3]) == 0x40000001 && word(two.hi[4 * 3 + 3]) == 0);
        const tier_data one = tiers_of(leaf_scene(5, medium_at(4, -1, -1)));
        CHECK(one.present && one.n_media_leaves == 1 && one.media_ord[0] == 4 && one.media_ord[1] == 0x7FFFFFFF);
        CHECK(no_tier_data(tiers_of(leaf_scene(5, medium_at(0, 2, 4)))));
    }
    {   // leaf 1 is instance 2, whose child is box 1, whose first face is quad 6: a lane tests the face, hi.w names the instance
        // (index + 1) and says "six faces" (bit 30).  Leaf 2 is box 0 itself (first face quad 0), leaf 3 instance 0 of a sphere.
        leaf_scene s(4, [](int q) { return q == 1 ? RT_PRIM_REF(RT_PRIM_INSTANCE, 2) : q == 2 ? RT_PRIM_REF(RT_PRIM_BOX, 0) : q == 3 ? RT_PRIM_REF(RT_PRIM_INSTANCE, 0) : sphere_q(q); });
        s.instances.resize(3);
        std::memset(s.instances.data(), 0, 3 * sizeof(rt_instance));
        s.instances[0].child = RT_PRIM_REF(RT_PRIM_SPHERE, 5); s.instances[1].child = RT_PRIM_REF(RT_PRIM_QUAD, 3); s.instances[2].child = RT_PRIM_REF(RT_PRIM_BOX, 1);
        s.boxes = {{0}, {6}};
        s.d.instances = s.instances.data(); s.d.n_instances = 3; s.d.boxes = s.boxes.data(); s.d.n_boxes = 2;
        const tier_data t = plan_tier_data(&s.d);
        CHECK(t.present && t.n_leaves == 4 && t.lo.size() == 256);
        if (t.lo.size() == 256) {
            CHECK(word(t.lo[4 * 1 + 3]) == 0x10000006 && word(t.hi[4 * 1 + 3]) == 0x40000003);
            CHECK(word(t.lo[4 * 2 + 3]) == 0x10000000 && word(t.hi[4 * 2 + 3]) == 0x40000000);
            CHECK(word(t.lo[4 * 3 + 3]) == 5 && word(t.hi[4 * 3 + 3]) == 1);
            CHECK(same_floats(&t.lo[4], {1, 0, 0}) && same_floats(&t.hi[4], {2, 1, 1}));   // the leaf's own box, not the child's
        }
    }
}

// ---- the checks of a description
// A description that passes: a root over three leaves -- sphere 0, instance 0 of box 0, medium 0 inside sphere 0 --, six quads, two
// materials, five textures (checker of solid and image, solid, a 2 x 2 image, noodle, uv_offset of the image) and 12 image bytes.
struct full_scene {
    std::vector<rt_node> nodes;
    std::vector<rt_sphere> spheres;
    std::vector<rt_quad> quads;
    std::vector<rt_box> boxes;
    std::vector<rt_instance> instances;
    std::vector<rt_medium> media;
    std::vector<rt_material> materials;
    std::vector<rt_texture> textures;
    std::vector<uint8_t> images;
    full_scene() {
        nodes = {bar(0, 4, 4, -1), bar(0, 1, 2, RT_PRIM_REF(RT_PRIM_SPHERE, 0)), bar(1, 2, 3, RT_PRIM_REF(RT_PRIM_INSTANCE, 0)), bar(2, 3, 4, RT_PRIM_REF(RT_PRIM_MEDIUM, 0))};
        spheres.resize(1); quads.resize(6); boxes.resize(1); instances.resize(1); media.resize(1); materials.resize(2); textures.resize(5);
        std::memset(spheres.data(), 0, sizeof(rt_sphere)); std::memset(quads.data(), 0, 6 * sizeof(rt_quad)); std::memset(instances.data(), 0, sizeof(rt_instance));
        std::memset(media.data(), 0, sizeof(rt_medium)); std::memset(materials.data(), 0, 2 * sizeof(rt_material)); std::memset(textures.data(), 0, 5 * sizeof(rt_texture));
        boxes[0].first_quad = 0;
        instances[0].child = RT_PRIM_REF(RT_PRIM_BOX, 0); instances[0].flags = RT_INST_TRANSLATE;
        media[0].boundary = RT_PRIM_REF(RT_PRIM_SPHERE, 0); media[0].mat = 1;
        materials[0].kind = RT_MAT_LAMBERTIAN; materials[0].tex = 0;
        materials[1].kind = RT_MAT_ISOTROPIC; materials[1].tex = -1;
        textures[0].kind = RT_TEX_CHECKER; textures[0].a = 1; textures[0].b = 2;
        textures[1].kind = RT_TEX_SOLID;
        textures[2].kind = RT_TEX_IMAGE; textures[2].a = 0; textures[2].b = 2; textures[2].c = 2;
        textures[3].kind = RT_TEX_NOODLE; textures[3].a = 4;
        textures[4].kind = RT_TEX_UV_OFFSET; textures[4].a = 2;
        images.assign(12, 0);
    }
    rt_scene_desc desc() const {
        rt_scene_desc d;
        std::memset(&d, 0, sizeof(d));
        d.nodes = nodes.data(); d.n_nodes = (int32_t)nodes.size(); d.spheres = spheres.data(); d.n_spheres = (int32_t)spheres.size();
        d.quads = quads.data(); d.n_quads = (int32_t)quads.size(); d.boxes = boxes.data(); d.n_boxes = (int32_t)boxes.size();
        d.instances = instances.data(); d.n_instances = (int32_t)instances.size(); d.media = media.data(); d.n_media = (int32_t)media.size();
        d.materials = materials.data(); d.n_materials = (int32_t)materials.size(); d.textures = textures.data(); d.n_textures = (int32_t)textures.size();
        d.images = images.data(); d.image_bytes = images.size();
        return d;
    }
};
// what validate says of the full scene after `change` (of the scene's arrays) and `change_desc` (of the description made of them)
template <class Change, class ChangeDesc> static bool refuses(const char* why, Change change, ChangeDesc change_desc) {
    full_scene s;
    change(s);
    rt_scene_desc d = s.desc();
    change_desc(d);
    scene_class cls;
    const char* got = validate(&d, cls);
    return got && std::strcmp(got, why) == 0;
}
template <class Change> static bool refuses(const char* why, Change change) { return refuses(why, change, [](rt_scene_desc&) {}); }
static void keep(full_scene&) {}
static bool is_class(const scene_class& c, bool spheres_only, int tex_level, bool need_uv) {
    return c.spheres_only == spheres_only && c.tex_level == tex_level && c.need_uv == need_uv;
}

static void check_validate() {
    scene_class cls;
    {
        const full_scene s;
        const rt_scene_desc d = s.desc();
        CHECK(validate(&d, cls) == nullptr && is_class(cls, false, 2, true));
    }
    const char* null_desc = validate(nullptr, cls);
    CHECK(null_desc && std::strcmp(null_desc, "null scene description") == 0);
    CHECK(refuses("negative count", keep, [](rt_scene_desc& d) { d.n_media = -1; }));
    CHECK(refuses("null array with non-zero count", keep, [](rt_scene_desc& d) { d.spheres = nullptr; }));
    CHECK(refuses("null array with non-zero count", keep, [](rt_scene_desc& d) { d.images = nullptr; }));
    CHECK(refuses("scene too large", keep, [](rt_scene_desc& d) { d.n_quads = 1 << 28; }));
    CHECK(refuses("node skip link does not move forward", [](full_scene& s) { s.nodes[2].skip = 2; }));
    CHECK(refuses("node skip link does not move forward", [](full_scene& s) { s.nodes[0].skip = 5; }));
    CHECK(refuses("medium index out of range", [](full_scene& s) { s.nodes[3].prim = RT_PRIM_REF(RT_PRIM_MEDIUM, 1); }));
    CHECK(refuses("leaf primitive reference out of range", [](full_scene& s) { s.nodes[1].prim = RT_PRIM_REF(RT_PRIM_SPHERE, 1); }));
    CHECK(refuses("leaf primitive reference out of range", [](full_scene& s) { s.nodes[1].prim = RT_PRIM_REF(5, 0); }));
    CHECK(refuses("sphere material out of range", [](full_scene& s) { s.spheres[0].mat = 2; }));
    CHECK(refuses("quad material out of range", [](full_scene& s) { s.quads[5].mat = -1; }));
    CHECK(refuses("box faces out of range", [](full_scene& s) { s.boxes[0].first_quad = 1; }));
    CHECK(refuses("instance child must be a sphere, quad or box", [](full_scene& s) { s.instances[0].child = RT_PRIM_REF(RT_PRIM_INSTANCE, 0); }));
    CHECK(refuses("medium boundary must be a sphere, quad, box or instance", [](full_scene& s) { s.media[0].boundary = RT_PRIM_REF(RT_PRIM_MEDIUM, 0); }));
    CHECK(refuses("medium material out of range", [](full_scene& s) { s.media[0].mat = 2; }));
    CHECK(refuses("unknown material kind", [](full_scene& s) { s.materials[1].kind = 5; }));
    CHECK(refuses("material texture out of range", [](full_scene& s) { s.materials[1].tex = 5; }));
    CHECK(refuses("checker child out of range", [](full_scene& s) { s.textures[0].b = 5; }));
    CHECK(refuses("checker children must be plain textures", [](full_scene& s) { s.textures[0].a = 4; }));
    CHECK(refuses("checker children must be plain textures", [](full_scene& s) { s.textures[0].b = 0; }));
    CHECK(refuses("image texture with non-positive size", [](full_scene& s) { s.textures[2].c = 0; }));
    CHECK(refuses("image texture outside the image pool", [](full_scene& s) { s.textures[2].a = 1; }));
    CHECK(refuses("noodle texture octaves out of range", [](full_scene& s) { s.textures[3].a = 17; }));
    CHECK(refuses("uv_offset child out of range", [](full_scene& s) { s.textures[4].a = -1; }));
    CHECK(refuses("uv_offset may wrap image, solid, noise, noodle or felt textures only", [](full_scene& s) { s.textures[4].a = 0; }));
    CHECK(refuses("unknown texture kind", [](full_scene& s) { s.textures[1].kind = 7; }));

    // the class: one leaf, one material whose texture (if any) is texture 0
    auto class_of = [](int32_t leaf_prim, int n_quads, int tex_kind) {
        const rt_node leaf = bar(0, 1, 1, leaf_prim);
        rt_sphere sphere; rt_quad quad; rt_material mat; rt_texture tex;
        std::memset(&sphere, 0, sizeof(sphere)); std::memset(&quad, 0, sizeof(quad)); std::memset(&mat, 0, sizeof(mat)); std::memset(&tex, 0, sizeof(tex));
        mat.tex = tex_kind < 0 ? -1 : 0;
        tex.kind = tex_kind; tex.a = -1;   // (an image with a < 0 names no bytes of the pool)
        rt_scene_desc d;
        std::memset(&d, 0, sizeof(d));
        d.nodes = &leaf; d.n_nodes = 1; d.spheres = &sphere; d.n_spheres = 1; d.quads = &quad; d.n_quads = n_quads;
        d.materials = &mat; d.n_materials = 1; d.textures = &tex; d.n_textures = tex_kind < 0 ? 0 : 1;
        scene_class c;
        CHECK(validate(&d, c) == nullptr);
        return c;
    };
    const int32_t a_sphere = RT_PRIM_REF(RT_PRIM_SPHERE, 0), a_quad = RT_PRIM_REF(RT_PRIM_QUAD, 0);
    CHECK(is_class(class_of(a_sphere, 0, -1), true, 0, false));               // spheres only
    CHECK(is_class(class_of(a_quad, 1, -1), false, 0, false));                // a quad
    CHECK(is_class(class_of(a_sphere, 1, -1), false, 0, false));              // ... even one no leaf holds
    CHECK(is_class(class_of(a_sphere, 0, RT_TEX_SOLID), true, 1, false));     // a plain texture
    CHECK(is_class(class_of(a_sphere, 0, RT_TEX_IMAGE), true, 2, true));      // an image texture
    CHECK(is_class(class_of(a_sphere, 0, RT_TEX_NOISE), true, 2, false));     // a noise texture: no uv
}

// ---- the marks on the copies creation uploads
// a quad whose unit normal (and w) is along axis c, with u and v on the two other axes
static rt_quad axis_quad(int c) {
    rt_quad q;
    std::memset(&q, 0, sizeof(q));
    q.n[c] = -1.0f; q.w[c] = 0.5f; q.u[(c + 1) % 3] = 2.0f; q.v[(c + 2) % 3] = -3.0f;
    q.pad0 = 77.0f;   // (whatever the description holds there is replaced)
    return q;
}
static void check_marks() {
    rt_scene_desc d;
    std::memset(&d, 0, sizeof(d));
    // box 0: faces along z, x, z, x, y, y (make_box's order); box 1: the first two swapped; then a tilted quad
    std::vector<rt_quad> quads;
    for (int c : {2, 0, 2, 0, 1, 1}) quads.push_back(axis_quad(c));
    for (int c : {0, 2, 2, 0, 1, 1}) quads.push_back(axis_quad(c));
    rt_quad tilted = axis_quad(2);
    tilted.n[1] = 0.6f; tilted.n[2] = 0.8f;
    quads.push_back(tilted);
    const rt_box boxes[2] = {{0}, {6}};
    d.quads = quads.data(); d.n_quads = 13; d.boxes = boxes; d.n_boxes = 2;
    const std::vector<rt_quad> mq = marked_quads(&d);
    CHECK(mq.size() == 13);
    if (mq.size() == 13) {
        const int32_t codes[13] = {3, 1, 3, 1, 2, 2, 1, 3, 3, 1, 2, 2, 0};   // 1 + axis; 0 for the tilted one
        for (int i = 0; i < 13; ++i) CHECK(word(mq[(size_t)i].pad0) == codes[i] && mq[(size_t)i].u[0] == quads[(size_t)i].u[0]);
    }
    const std::vector<rt_box> mb = marked_boxes(&d);
    CHECK(mb.size() == 2 && mb[0].first_quad == 0x40000000 && mb[1].first_quad == 6);

    // textures: 0 checker of (solid 1, image 2), 1 solid, 2 image, 3 noise, 4 checker of (solid 1, solid 1), 5 uv_offset of 3
    rt_texture tex[6];
    std::memset(tex, 0, sizeof(tex));
    tex[0].kind = RT_TEX_CHECKER; tex[0].a = 1; tex[0].b = 2;
    tex[1].kind = RT_TEX_SOLID; tex[2].kind = RT_TEX_IMAGE; tex[3].kind = RT_TEX_NOISE;
    tex[4].kind = RT_TEX_CHECKER; tex[4].a = 1; tex[4].b = 1;
    tex[5].kind = RT_TEX_UV_OFFSET; tex[5].a = 3;
    rt_material mats[7];
    std::memset(mats, 0, sizeof(mats));
    const int32_t of[7] = {0, -1, 1, 2, 3, 4, 5};
    for (int i = 0; i < 7; ++i) { mats[i].tex = of[i]; mats[i].pad = 9.0f; mats[i].fuzz = (float)i; }
    d.textures = tex; d.n_textures = 6; d.materials = mats; d.n_materials = 7;
    const std::vector<rt_material> mm = marked_materials(&d);
    CHECK(mm.size() == 7);
    if (mm.size() == 7) {
        const float reads_uv[7] = {1, 0, 0, 1, 0, 0, 1};   // the checker with an image child, no texture, solid, image, noise, a plain checker, uv_offset
        for (int i = 0; i < 7; ++i) CHECK(mm[(size_t)i].pad == reads_uv[i] && mm[(size_t)i].fuzz == (float)i && mm[(size_t)i].tex == of[i]);
    }

    // the bound: the largest |coordinate| per axis over every node
    const rt_node nodes[2] = {node(-3, 1, -7, 2, 5, -6, 2, -1), node(0, -9, 0, 4, 0, 1, 2, 0)};
    float bound[3] = {-1, -1, -1};
    axis_bound(nodes, 2, bound);
    CHECK(bound[0] == 4.0f && bound[1] == 9.0f && bound[2] == 7.0f);
    axis_bound(nullptr, 0, bound);
    CHECK(bound[0] == 0.0f && bound[1] == 0.0f && bound[2] == 0.0f);
}

int main() {
    check_collapse_two_leaves();
    check_collapse_middle_dropped();
    check_collapse_leaves_alone();
    check_regroup();
    check_scanned_and_encoding();
    check_tier_data();
    check_validate();
    check_marks();
    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("scene plan ok\n");
    return 0;
}
