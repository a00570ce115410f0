// rt_scene_plan.h -- what rt_scene_create decides before its first upload (rt_abi.hip): the checks of
// a description and the scene's class, the walk-array planner ("Collapse"), the regrouped hierarchies ("Regroup"), the leaves-only
// array of a scanned scene, the device's link encoding, the tier data and the marked copies of quads, boxes and materials.  Host
// only and plain C++: no HIP call, no global, no scene; every function reads a description or a node array and returns a value.
// rt_abi.hip uploads what these return; tests/scene_plan_check.cpp checks the rules here on a CPU.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <utility>
#include <vector>

#include "../../include/rt_abi.h"
#include "rt_refit_host.h"

namespace rt_scene_plan {

// ---- the checks of a description

inline bool simple_ref_ok(const rt_scene_desc* d, int32_t ref) {
    if (ref < 0) return false;
    const int k = RT_PRIM_KIND(ref), i = RT_PRIM_INDEX(ref);
    if (k == RT_PRIM_SPHERE) return i < d->n_spheres;
    if (k == RT_PRIM_QUAD) return i < d->n_quads;
    if (k == RT_PRIM_BOX) return i < d->n_boxes;
    return false;
}
inline bool solid_ref_ok(const rt_scene_desc* d, int32_t ref) {
    if (ref < 0) return false;
    if (RT_PRIM_KIND(ref) == RT_PRIM_INSTANCE) return RT_PRIM_INDEX(ref) < d->n_instances;
    return simple_ref_ok(d, ref);
}

// what picks a scene's kernel family: every leaf a sphere and no other primitive array; 0 = no texture, 1 = solid and checker
// textures, 2 = noise, image or uv_offset ones; some texture reads the hit's (u, v)
struct scene_class {
    bool spheres_only = false;
    int tex_level = 0;
    bool need_uv = false;
};

// Every index a kernel will follow is checked here, on the host, so that a malformed description is an error code and never a
// GPU fault.  Returns why the description is refused (tests and the Python layer match on the words), or null and its class.
inline const char* validate(const rt_scene_desc* d, scene_class& cls) {
    if (!d) return "null scene description";
    if (d->n_nodes < 0 || d->n_spheres < 0 || d->n_quads < 0 || d->n_boxes < 0 || d->n_instances < 0 || d->n_media < 0 ||
        d->n_materials < 0 || d->n_textures < 0)
        return "negative count";
    if ((d->n_nodes && !d->nodes) || (d->n_spheres && !d->spheres) || (d->n_quads && !d->quads) || (d->n_boxes && !d->boxes) ||
        (d->n_instances && !d->instances) || (d->n_media && !d->media) || (d->n_materials && !d->materials) ||
        (d->n_textures && !d->textures) || (d->image_bytes && !d->images))
        return "null array with non-zero count";
    if (d->n_nodes >= (1 << 28) || d->n_spheres >= (1 << 28) || d->n_quads >= (1 << 28)) return "scene too large";
    cls = scene_class();
    cls.spheres_only = !(d->n_quads || d->n_boxes || d->n_instances || d->n_media);
    for (int i = 0; i < d->n_nodes; ++i) {
        const rt_node& n = d->nodes[i];
        if (n.skip <= i || n.skip > d->n_nodes) return "node skip link does not move forward";
        if (n.prim >= 0) {
            const int k = RT_PRIM_KIND(n.prim), idx = RT_PRIM_INDEX(n.prim);
            if (k != RT_PRIM_SPHERE) cls.spheres_only = false;
            if (k == RT_PRIM_MEDIUM) { if (idx >= d->n_media) return "medium index out of range"; }
            else if (!solid_ref_ok(d, n.prim)) return "leaf primitive reference out of range";
        }
    }
    for (int i = 0; i < d->n_spheres; ++i)
        if (d->spheres[i].mat < 0 || d->spheres[i].mat >= d->n_materials) return "sphere material out of range";
    for (int i = 0; i < d->n_quads; ++i)
        if (d->quads[i].mat < 0 || d->quads[i].mat >= d->n_materials) return "quad material out of range";
    for (int i = 0; i < d->n_boxes; ++i)
        if (d->boxes[i].first_quad < 0 || d->boxes[i].first_quad + 6 > d->n_quads) return "box faces out of range";
    for (int i = 0; i < d->n_instances; ++i)
        if (!simple_ref_ok(d, d->instances[i].child)) return "instance child must be a sphere, quad or box";
    for (int i = 0; i < d->n_media; ++i) {
        if (!solid_ref_ok(d, d->media[i].boundary)) return "medium boundary must be a sphere, quad, box or instance";
        if (d->media[i].mat < 0 || d->media[i].mat >= d->n_materials) return "medium material out of range";
    }
    for (int i = 0; i < d->n_materials; ++i) {
        const rt_material& m = d->materials[i];
        if (m.kind < RT_MAT_LAMBERTIAN || m.kind > RT_MAT_ISOTROPIC) return "unknown material kind";
        if (m.tex >= d->n_textures) return "material texture out of range";
        if (m.tex >= 0 && cls.tex_level < 1) cls.tex_level = 1;
    }
    for (int i = 0; i < d->n_textures; ++i) {
        const rt_texture& t = d->textures[i];
        if (t.kind == RT_TEX_CHECKER) {
            // even/odd must point at later-or-earlier non-self entries that terminate: forbid checker children
            if (t.a < 0 || t.a >= d->n_textures || t.b < 0 || t.b >= d->n_textures) return "checker child out of range";
            if (d->textures[t.a].kind == RT_TEX_CHECKER || d->textures[t.b].kind == RT_TEX_CHECKER ||
                d->textures[t.a].kind == RT_TEX_UV_OFFSET || d->textures[t.b].kind == RT_TEX_UV_OFFSET)
                return "checker children must be plain textures";
        } else if (t.kind == RT_TEX_IMAGE) {
            cls.need_uv = true; cls.tex_level = 2;
            if (t.a >= 0) {
                if (t.b <= 0 || t.c <= 0) return "image texture with non-positive size";
                if ((size_t)t.a + (size_t)t.b * t.c * 3 > d->image_bytes) return "image texture outside the image pool";
            }
        } else if (t.kind == RT_TEX_NOISE || t.kind == RT_TEX_NOODLE || t.kind == RT_TEX_FELT) {
            cls.tex_level = 2;
            if (t.kind == RT_TEX_NOODLE && (t.a < 0 || t.a > 16)) return "noodle texture octaves out of range";
        } else if (t.kind == RT_TEX_UV_OFFSET) {
            cls.tex_level = 2; cls.need_uv = true;
            if (t.a < 0 || t.a >= d->n_textures) return "uv_offset child out of range";
            if (d->textures[t.a].kind == RT_TEX_UV_OFFSET || d->textures[t.a].kind == RT_TEX_CHECKER)
                return "uv_offset may wrap image, solid, noise, noodle or felt textures only";
        } else if (t.kind != RT_TEX_SOLID) {
            return "unknown texture kind";
        }
    }
    return nullptr;
}

// ---------------------------------------------------------------------------------------------------------------
// "Collapse": which interior nodes of the reference's tree are worth testing.
//
// bvh_node::hit (bvh.cuh:95-106) reaches an object iff every ancestor box and the object's own box (its single-object
// node, bvh.cuh:38-43) pass against the closest hit so far.  The slab test (aabb.cuh:45-61) is monotone in the box (a
// box containing another is entered no later and left no earlier, rounding included: the same subtract-multiply on
// ordered operands; a NaN from 0 * inf leaves a limit unconstrained for parent and child alike) and in the limit, and
// limits only shrink during a walk.  So "the own box passes at the moment of the object test" already implies every
// ancestor passed earlier: the interior boxes never change a result, they only save work -- and only if they fail
// often enough.  Dropping interior node X (its children take its place in the depth-first array) removes one test per
// visit of X and adds one failing test per direct child whenever X would have failed; with v = visits and p = passes
// that is a saving iff p / v > 1 - 1 / k.  A median-split tree has many such nodes (the random scene: 40.1 -> 29.4 box
// tests per ray, Cornell 14.6 -> 8.6, Book-2 final 55.1 -> 35.6).  The choice is an exact tree DP over (node, nearest
// kept ancestor) on pass counts -- measured by kernel 0 on a small frame of the scene's own camera (bvh_collapse = 2),
// or taken proportional to box surface area (1).  Order of the leaves, every leaf node and every box value are the
// reference's; frames are bit-identical with the option on or off (tests/test_gpu_parity.py).
// ---------------------------------------------------------------------------------------------------------------
struct collapse_plan {
    std::vector<char> keep;     // per reference node
    double tests_before = 0, tests_after = 0;   // expected box tests per calibration ray
};

// The pass counts of a tree nobody measured: a ray that passes a box passes a box inside it about in proportion to the surface
// areas.  The root's figure stands for the visits of the root.
inline std::vector<double> area_passes(const rt_node* nodes, int n) {
    std::vector<double> pass((size_t)n, 0.0);
    for (int i = 0; i < n; ++i) {
        const double ex = fmax(0.0, (double)nodes[i].bmax[0] - nodes[i].bmin[0]), ey = fmax(0.0, (double)nodes[i].bmax[1] - nodes[i].bmin[1]),
                     ez = fmax(0.0, (double)nodes[i].bmax[2] - nodes[i].bmin[2]);
        pass[(size_t)i] = 2.0 * (ex * ey + ey * ez + ex * ez);
    }
    return pass;
}

// children of interior node i in the depth-first array: i + 1, then each next sibling at the previous one's skip link
template <class F> inline void for_children(const rt_node* nodes, int i, F f) {
    for (int c = i + 1; c < nodes[i].skip; c = nodes[c].skip) f(c);
}

// Returns whether the tree was planned; one that was not (too small, too deep, not a tree of nested boxes) is walked as given:
// every node kept.  The skip links are the caller's to have checked (validate: forward, inside the array).
inline bool plan_collapse(const rt_node* nodes, int n, const std::vector<double>& pass, double root_visits, collapse_plan& plan) {
    plan.keep.assign((size_t)n, 1);
    if (n < 3 || root_visits <= 0) return false;
    // depth of every node (= length of its ancestor chain); parents precede children in the array
    std::vector<int> depth((size_t)n, 0), parent((size_t)n, -1);
    int max_depth = 0;
    for (int i = 0; i < n; ++i)
        if (nodes[i].prim < 0) for_children(nodes, i, [&](int c) { depth[c] = depth[i] + 1; parent[c] = i; if (depth[c] > max_depth) max_depth = depth[c]; });
    if (max_depth > 60) return false;   // a degenerate (list-like) tree: leave it alone
    // the argument above needs a real tree (children tile their parent's range of the array) whose boxes contain their
    // children's; a description that is anything else is walked as given
    for (int i = 0; i < n; ++i) {
        if (i > 0 && parent[i] < 0) return false;
        if (nodes[i].prim >= 0) { if (nodes[i].skip != i + 1) return false; continue; }
        int c = i + 1, kids = 0;
        for (; c < nodes[i].skip; c = nodes[c].skip) {
            ++kids;
            for (int a = 0; a < 3; ++a)
                if (!(nodes[c].bmin[a] >= nodes[i].bmin[a] && nodes[c].bmax[a] <= nodes[i].bmax[a])) return false;
        }
        if (c != nodes[i].skip || kids == 0) return false;
    }
    // cost[i][d]: fewest tests in the subtree of i per calibration run when the nearest kept ancestor is the d-th entry of
    // i's ancestor chain (0 = "above the root": root_visits, 1.. = ancestors from the root down); visits of a node = passes
    // of its nearest kept ancestor (a fixed-order walk has no other way to skip it)
    std::vector<std::vector<double>> cost((size_t)n);
    auto visits = [&](int i, int d) -> double {   // d-th entry of i's chain
        if (d == 0) return root_visits;
        int a = i;
        for (int up = depth[i] - d + 1; up > 0; --up) a = parent[a];
        return pass[a];
    };
    for (int i = n - 1; i >= 0; --i) {   // children have larger indices: reverse order is post-order enough
        const int D = depth[i] + 1;
        cost[i].assign((size_t)D, 0.0);
        if (nodes[i].prim >= 0) { for (int d = 0; d < D; ++d) cost[i][d] = visits(i, d); continue; }
        for (int d = 0; d < D; ++d) {
            double keep = visits(i, d), drop = 0.0;
            for_children(nodes, i, [&](int c) { keep += cost[c][(size_t)D]; drop += cost[c][(size_t)d]; });
            cost[i][d] = keep <= drop ? keep : drop;
        }
    }
    // decide top-down
    std::vector<int> nearest((size_t)n, 0);
    double before = 0.0;
    for (int i = 0; i < n; ++i) before += (i == 0) ? root_visits : pass[parent[i]];
    for (int i = 0; i < n; ++i) {
        const int d = nearest[i];
        bool keep = true;
        if (nodes[i].prim < 0) {
            double k = visits(i, d), drop = 0.0;
            const int D = depth[i] + 1;
            for_children(nodes, i, [&](int c) { k += cost[c][(size_t)D]; drop += cost[c][(size_t)d]; });
            keep = k <= drop;
            for_children(nodes, i, [&](int c) { nearest[c] = keep ? D : d; });
        }
        plan.keep[i] = keep ? 1 : 0;
    }
    plan.tests_before = before / root_visits;
    plan.tests_after = cost[0][0] / root_visits;
    return true;
}

// the walk array: kept nodes in the reference's depth-first order, skip links re-pointed at the next kept node
inline std::vector<rt_node> build_walk_array(const rt_node* nodes, int n, const std::vector<char>& keep) {
    std::vector<int> kept_before((size_t)n + 1, 0);
    for (int i = 0; i < n; ++i) kept_before[i + 1] = kept_before[i] + (keep[i] ? 1 : 0);
    std::vector<rt_node> walk;
    walk.reserve((size_t)kept_before[n]);
    for (int i = 0; i < n; ++i) {
        if (!keep[i]) continue;
        rt_node w = nodes[i];
        w.skip = kept_before[nodes[i].skip];
        walk.push_back(w);
    }
    return walk;
}

// ---------------------------------------------------------------------------------------------------------------
// "Regroup": another hierarchy over the same leaves.
//
// By the argument above the walk returns what the reference's returns as long as (1) the leaves -- the reference's
// single-object nodes, with their boxes -- come in the reference's depth-first order and (2) every interior box contains
// the boxes below it: then "a leaf's own box passes" still implies that everything above it passed, and a subtree is
// only ever skipped when none of its leaves could have passed.  Which contiguous runs of leaves are grouped is free.  The
// reference groups by halving (bvh.cuh:25-36), which puts a huge object (the ground sphere: a 2000-unit box) into half of
// the top of the tree: every box above it is as large as it is and always passes.  regroup_leaves() builds a binary tree
// over the same leaf sequence, interior boxes = the exact union (float min / max) of their leaves' boxes, in one of two
// ways: top-down -- split [a, b) at the k that minimises area(a..k) * (k - a) + area(k..b) * (b - k) -- or bottom-up --
// keep merging the two neighbouring groups with the smallest union, "smallest" by surface area (method 1) or by how many
// of ~4000 rays sampled from the calibration pass meet it (method 2: the scene as this camera's paths see it).  Each goes
// through the same calibration pass and collapse DP as the reference's tree, and whichever walk array predicts the fewest
// box tests per ray is used (bvh_collapse = 3).
// ---------------------------------------------------------------------------------------------------------------
struct box { float lo[3], hi[3]; };
const box EMPTY_BOX = {{FLT_MAX, FLT_MAX, FLT_MAX}, {-FLT_MAX, -FLT_MAX, -FLT_MAX}};
inline void grow(box& b, const rt_node& l) { for (int a = 0; a < 3; ++a) { b.lo[a] = fminf(b.lo[a], l.bmin[a]); b.hi[a] = fmaxf(b.hi[a], l.bmax[a]); } }
inline box unite(const box& x, const box& y) { box u = x; for (int a = 0; a < 3; ++a) { u.lo[a] = fminf(u.lo[a], y.lo[a]); u.hi[a] = fmaxf(u.hi[a], y.hi[a]); } return u; }
inline double area(const box& b) {
    const double x = fmax(0.0, (double)b.hi[0] - b.lo[0]), y = fmax(0.0, (double)b.hi[1] - b.lo[1]), z = fmax(0.0, (double)b.hi[2] - b.lo[2]);
    return 2.0 * (x * y + y * z + x * z);
}

// The depth-first array both builders write, a node at a time in pre-order: an interior node says how many leaves lie below
// it, and its skip link is patched when the last of them has come.
struct depth_first_emitter {
    std::vector<rt_node> out;
    std::vector<std::pair<int, int>> open;   // (index of an interior node, number of leaves still to be emitted under it)
    void interior(const box& b, int leaves_below) {
        rt_node nd;
        for (int a = 0; a < 3; ++a) { nd.bmin[a] = b.lo[a]; nd.bmax[a] = b.hi[a]; }
        nd.prim = -1; nd.skip = 0;
        open.push_back({(int)out.size(), leaves_below});
        out.push_back(nd);
    }
    void leaf(rt_node l) {
        l.skip = (int32_t)out.size() + 1;
        out.push_back(l);
        // every enclosing interior node has one leaf fewer to wait for; those that are complete end here
        for (auto& o : open) --o.second;
        while (!open.empty() && open.back().second == 0) { out[(size_t)open.back().first].skip = (int32_t)out.size(); open.pop_back(); }
    }
};

// top-down: split [a, b) at the k that minimises area(a..k) * (k - a) + area(k..b) * (b - k); the middle where no cost is finite
inline std::vector<rt_node> split_top_down(const std::vector<rt_node>& leaves) {
    const int m = (int)leaves.size();
    depth_first_emitter emit;
    emit.out.reserve((size_t)(2 * m));
    std::vector<double> right_area((size_t)m + 1);
    struct range { int a, b; };
    std::vector<range> todo;   // explicit stack: ranges in depth-first order
    todo.push_back({0, m});
    while (!todo.empty()) {
        const range it = todo.back();
        todo.pop_back();
        if (it.b - it.a == 1) { emit.leaf(leaves[(size_t)it.a]); continue; }
        box all = EMPTY_BOX;
        for (int k = it.a; k < it.b; ++k) grow(all, leaves[(size_t)k]);
        // areas of the right parts [k, b), then sweep the left part
        box r = EMPTY_BOX;
        for (int k = it.b - 1; k > it.a; --k) { grow(r, leaves[(size_t)k]); right_area[(size_t)k] = area(r); }
        box l = EMPTY_BOX;
        int best_k = (it.a + it.b) / 2;
        double best = -1.0;
        for (int k = it.a + 1; k < it.b; ++k) {
            grow(l, leaves[(size_t)k - 1]);
            const double c = area(l) * (double)(k - it.a) + right_area[(size_t)k] * (double)(it.b - k);
            if (std::isfinite(c) && (best < 0.0 || c < best)) { best = c; best_k = k; }
        }
        emit.interior(all, it.b - it.a);
        todo.push_back({best_k, it.b});      // right part second
        todo.push_back({it.a, best_k});      // left part first
    }
    return emit.out;
}

// The sampled rays of a calibration pass (seven floats a ray: origin, direction, the limit it ended with) as seven arrays --
// origin, 1 / direction, limit -- so that the loop of seen_by vectorises: a scene's creation time depends on it.
struct ray_sample {
    std::vector<float> q[7];
    size_t n_rays = 0;
    explicit ray_sample(const std::vector<float>* sample) {
        n_rays = sample ? sample->size() / 7 : 0;
        for (int a = 0; a < 7; ++a) q[a].resize(n_rays);
        for (size_t r = 0; r < n_rays; ++r) {
            for (int a = 0; a < 3; ++a) { q[a][r] = (*sample)[r * 7 + a]; q[3 + a][r] = 1.0f / (*sample)[r * 7 + 3 + a]; }
            q[6][r] = (*sample)[r * 7 + 6];
        }
    }
    // how many of the rays pass the box, each with the limit it ended with (the kernels' slab test from 0.001)
    double seen_by(const box& b) const {
        unsigned int hits = 0;
        for (size_t r = 0; r < n_rays; ++r) {
            float t0 = 0.001f, t1 = q[6][r];
            for (int a = 0; a < 3; ++a) {
                const float x = (b.lo[a] - q[a][r]) * q[3 + a][r], y = (b.hi[a] - q[a][r]) * q[3 + a][r];
                const float lo_t = x < y ? x : y, hi_t = x < y ? y : x;
                t0 = lo_t > t0 ? lo_t : t0;
                t1 = hi_t < t1 ? hi_t : t1;
            }
            hits += (t1 <= t0) ? 0u : 1u;
        }
        return (double)hits;
    }
};

// The merger's two keys of a union box, smaller = merged sooner: its surface area, or -- with sampled rays -- the rays that
// meet it first and the area, squashed below one ray, second.  A non-finite area comes last either way.
inline double area_key(const box& u) { const double ar = area(u); return std::isfinite(ar) ? ar : DBL_MAX; }
inline double sampled_ray_key(const box& u, const ray_sample& rays) {
    const double ar = area(u);
    return std::isfinite(ar) ? rays.seen_by(u) + ar / (ar + 1.0) : DBL_MAX;
}

// bottom-up: merge, again and again, the two neighbouring groups whose union has the smallest key (a heap of neighbour pairs
// with lazy deletion; ties go to the pair further left); a huge leaf is merged last and ends up directly under the root.
template <class Key> inline std::vector<rt_node> merge_bottom_up(const std::vector<rt_node>& leaves, Key key) {
    const int m = (int)leaves.size();
    struct group { box b; int left, right, leaf, prev, next, count; bool alive; };
    std::vector<group> g((size_t)m);
    for (int i = 0; i < m; ++i) {
        g[(size_t)i].b = EMPTY_BOX; grow(g[(size_t)i].b, leaves[(size_t)i]);
        g[(size_t)i].left = g[(size_t)i].right = -1; g[(size_t)i].leaf = i; g[(size_t)i].prev = i - 1; g[(size_t)i].next = i + 1 < m ? i + 1 : -1;
        g[(size_t)i].count = 1; g[(size_t)i].alive = true;
    }
    struct pair_key { double key; int i, j; };
    auto worse = [](const pair_key& x, const pair_key& y) { return x.key > y.key || (x.key == y.key && x.i > y.i); };
    std::vector<pair_key> heap;
    auto push = [&](int i, int j) {
        heap.push_back({key(unite(g[(size_t)i].b, g[(size_t)j].b)), i, j});
        std::push_heap(heap.begin(), heap.end(), worse);
    };
    for (int i = 0; i + 1 < m; ++i) push(i, i + 1);
    int root = m - 1;
    while (!heap.empty()) {
        std::pop_heap(heap.begin(), heap.end(), worse);
        const pair_key k = heap.back();
        heap.pop_back();
        if (!g[(size_t)k.i].alive || !g[(size_t)k.j].alive) continue;
        group u;
        u.b = unite(g[(size_t)k.i].b, g[(size_t)k.j].b); u.left = k.i; u.right = k.j; u.leaf = -1;
        u.prev = g[(size_t)k.i].prev; u.next = g[(size_t)k.j].next; u.count = g[(size_t)k.i].count + g[(size_t)k.j].count; u.alive = true;
        g[(size_t)k.i].alive = g[(size_t)k.j].alive = false;
        const int id = (int)g.size();
        g.push_back(u);
        root = id;
        if (u.prev >= 0) { g[(size_t)u.prev].next = id; push(u.prev, id); }
        if (u.next >= 0) { g[(size_t)u.next].prev = id; push(id, u.next); }
    }
    depth_first_emitter emit;
    emit.out.reserve((size_t)(2 * m));
    std::vector<int> todo;
    todo.push_back(root);
    while (!todo.empty()) {
        const int id = todo.back();
        todo.pop_back();
        if (g[(size_t)id].leaf >= 0) { emit.leaf(leaves[(size_t)g[(size_t)id].leaf]); continue; }
        emit.interior(g[(size_t)id].b, g[(size_t)id].count);
        todo.push_back(g[(size_t)id].right);
        todo.push_back(g[(size_t)id].left);
    }
    return emit.out;
}

// method 0 = top-down, 1 = bottom-up by area, 2 = bottom-up by the sampled rays (by area where `sample` holds no ray)
inline std::vector<rt_node> regroup_leaves(const rt_node* nodes, int n, int method, const std::vector<float>* sample = nullptr) {
    std::vector<rt_node> leaves;
    for (int i = 0; i < n; ++i) if (nodes[i].prim >= 0) leaves.push_back(nodes[i]);
    if (leaves.empty()) return leaves;
    if (method < 1) return split_top_down(leaves);
    const ray_sample rays(method == 2 ? sample : nullptr);
    if (!rays.n_rays) return merge_bottom_up(leaves, area_key);
    return merge_bottom_up(leaves, [&](const box& u) { return sampled_ray_key(u, rays); });
}

// A walk array this small is not walked but scanned in lockstep (lds_mode 4; option scan_nodes): every lane of a wave steps
// through every node whatever its own boxes said, so an interior node can only cost.  The leaves alone, in their order, are the
// array then (the Cornell box: 11 -> 10 nodes).  Returns whether `walk` was replaced.
inline bool leaves_only_if_scanned(const rt_node* src, int m, int scan_nodes, std::vector<rt_node>& walk) {
    if (scan_nodes <= 0 || m > scan_nodes) return false;
    std::vector<rt_node> leaves;
    for (int i = 0; i < m; ++i)
        if (src[i].prim >= 0) { rt_node w = src[i]; w.skip = (int32_t)leaves.size() + 1; leaves.push_back(w); }
    if (leaves.empty() || (int)leaves.size() >= m) return false;
    walk.swap(leaves);
    return true;
}

// A node array in the device's link encoding (rt_device.h, RT_NODE_SKIP): `skip` holds ~skip, `prim` holds ~(own index + 1) at
// an interior node (still < 0) and stays the object reference (>= 0) at a leaf.
inline std::vector<rt_node> device_nodes(const rt_node* nodes, size_t n) {
    std::vector<rt_node> out(nodes, nodes + n);
    for (size_t i = 0; i < n; ++i) {
        out[i].skip = ~out[i].skip;
        if (out[i].prim < 0) out[i].prim = ~(int32_t)(i + 1);
    }
    return out;
}

// Tier data (rt_kernel_tier.h): the scene's leaves -- the reference's single-object nodes, in its depth-first order, which
// every walk array keeps -- as two float4 arrays padded to whole 64-leaf slots, and per slot the union of its boxes (eight
// floats: lo, hi, two unused).  A scene with no leaf, more than 64 slots (one lane tests one slot's union) or more than two
// constant_medium leaves gets none (`present` unset, everything else as constructed): it renders without a tier kernel.
struct tier_data {
    bool present = false;
    std::vector<float> lo, hi, ranges;
    int n_leaves = 0, n_slots = 0, n_media_leaves = 0;
    int media_ord[2] = {0x7FFFFFFF, 0x7FFFFFFF};   // the leaf ordinals of the media
};
inline tier_data plan_tier_data(const rt_scene_desc* d) {
    std::vector<const rt_node*> leaves;
    for (int i = 0; i < d->n_nodes; ++i) if (d->nodes[i].prim >= 0) leaves.push_back(&d->nodes[i]);
    const int m = (int)leaves.size();
    if (m == 0 || m > 64 * 64) return tier_data();
    tier_data t;
    for (int q = 0; q < m; ++q)
        if (RT_PRIM_KIND(leaves[q]->prim) == RT_PRIM_MEDIUM) { if (t.n_media_leaves < 2) t.media_ord[t.n_media_leaves] = q; ++t.n_media_leaves; }
    if (t.n_media_leaves > 2) return tier_data();
    const int slots = (m + 63) / 64;
    t.lo.resize((size_t)slots * 64 * 4); t.hi.resize((size_t)slots * 64 * 4); t.ranges.assign((size_t)slots * 8, 0.0f);
    for (int k = 0; k < slots; ++k) {
        float rl[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, rh[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
        for (int l = 0; l < 64; ++l) {
            const int q = k * 64 + l;
            float* a = &t.lo[(size_t)q * 4];
            float* b = &t.hi[(size_t)q * 4];
            // lo.w = what a lane tests: the leaf's sphere or quad, for a box (compound6, quad.cuh:124-139) its FIRST face, for an
            // instance the same of its child; a medium stays itself.  hi.w = instance index + 1 (0 = none) | bit 30: "six faces
            // from lo.w on" (rt_kernel_tier.h shares those out over six lanes)
            int32_t prim = -1, xw = 0;
            if (q < m) {
                for (int c = 0; c < 3; ++c) { a[c] = leaves[q]->bmin[c]; b[c] = leaves[q]->bmax[c]; rl[c] = fminf(rl[c], a[c]); rh[c] = fmaxf(rh[c], b[c]); }
                prim = leaves[q]->prim;
                if (RT_PRIM_KIND(prim) == RT_PRIM_INSTANCE) {
                    const int idx = RT_PRIM_INDEX(prim);
                    if (idx >= d->n_instances || idx >= (1 << 29)) return tier_data();   // (validate has checked the refs; no tier data otherwise)
                    xw = idx + 1;
                    prim = d->instances[idx].child;
                }
                if (RT_PRIM_KIND(prim) == RT_PRIM_BOX) {
                    const int idx = RT_PRIM_INDEX(prim);
                    if (idx >= d->n_boxes) return tier_data();
                    prim = RT_PRIM_REF(RT_PRIM_QUAD, d->boxes[idx].first_quad & 0x3FFFFFFF);
                    xw |= 1 << 30;
                }
            } else {
                for (int c = 0; c < 3; ++c) { a[c] = 0.0f; b[c] = 0.0f; }
            }
            memcpy(&a[3], &prim, 4);
            memcpy(&b[3], &xw, 4);
        }
        for (int c = 0; c < 3; ++c) { t.ranges[(size_t)k * 8 + c] = rl[c]; t.ranges[(size_t)k * 8 + 3 + c] = rh[c]; }
    }
    t.present = true;
    t.n_leaves = m; t.n_slots = slots;
    return t;
}

// ---- the derived copies creation uploads in place of the description's arrays

// Quads and boxes with the axis-aligned ones marked (quad_test_axis, rt_device_funcs.h).  A quad qualifies when its unit normal
// is exactly +-e_C and u, v, w each have exactly one non-zero component on the fitting axes: its code goes to pad0.  A box
// qualifies when its six faces do, with normals along z, x, z, x, y, y (make_box's order, quad.cuh:145-162): bit 30 of
// first_quad.  Both rules live in rt_refit_host.h, where rt_scene_update_quads takes them from too.
inline std::vector<rt_quad> marked_quads(const rt_scene_desc* d) {
    std::vector<rt_quad> quads(d->quads, d->quads + d->n_quads);
    for (rt_quad& q : quads) { const int32_t code = rt_refit::axis_code(q); memcpy(&q.pad0, &code, 4); }
    return quads;
}
inline std::vector<rt_box> marked_boxes(const rt_scene_desc* d) {
    std::vector<rt_box> boxes(d->boxes, d->boxes + d->n_boxes);
    for (rt_box& b : boxes) {
        int32_t codes[6];
        for (int f = 0; f < 6; ++f) codes[f] = rt_refit::axis_code(d->quads[(size_t)b.first_quad + f]);
        if (rt_refit::canonical_codes(codes)) b.first_quad |= RT_BOX_CANONICAL;
    }
    return boxes;
}
// materials: `pad` tells resolve_hit() whether the material's texture reads the hit's (u, v)
inline std::vector<rt_material> marked_materials(const rt_scene_desc* d) {
    std::vector<rt_material> mats(d->materials, d->materials + d->n_materials);
    auto reads_uv = [&](int tex) -> bool {
        if (tex < 0) return false;
        const rt_texture& t = d->textures[tex];
        if (t.kind == RT_TEX_IMAGE || t.kind == RT_TEX_UV_OFFSET) return true;
        if (t.kind == RT_TEX_CHECKER) {
            const int ka = d->textures[t.a].kind, kb = d->textures[t.b].kind;   // validate: checker children are plain textures
            return ka == RT_TEX_IMAGE || kb == RT_TEX_IMAGE;
        }
        return false;
    };
    for (rt_material& m : mats) m.pad = reads_uv(m.tex) ? 1.0f : 0.0f;
    return mats;
}
// the scene's coordinate bound per axis (regrouped interior boxes are unions of the description's: the same bound)
inline void axis_bound(const rt_node* nodes, int n, float bound[3]) {
    for (int c = 0; c < 3; ++c) {
        float b = 0.0f;
        for (int i = 0; i < n; ++i) b = fmaxf(b, fmaxf(fabsf(nodes[i].bmin[c]), fabsf(nodes[i].bmax[c])));
        bound[c] = b;
    }
}

}  // namespace rt_scene_plan
