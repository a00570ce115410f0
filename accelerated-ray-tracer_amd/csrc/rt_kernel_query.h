// rt_kernel_query.h -- what the query kernels share (rt_kernel_trace.hip, rt_kernel_radiance.hip, rt_kernel_aov.hip,
// rt_kernel_aov_through.hip): the test that a ray can be walked, the start of a walk and its node visit.  Each of those kernels
// keeps one ray per lane and runs one node visit per trip of its loop.  Internal to librt_mi355x.so.
#pragma once
#include "rt_device_funcs.h"

namespace {

// every component of the ray finite: quad_test and medium_test would accept a NaN t, and the box forms disagree on NaN
// (fminf / fmaxf drop it, the ternaries keep it), so the walk taken would decide the answer -- such a ray is not walked
DEV bool ray_is_finite(const Ray& r) {
    return isfinite(r.o.x) && isfinite(r.o.y) && isfinite(r.o.z) && isfinite(r.d.x) && isfinite(r.d.y) && isfinite(r.d.z) && isfinite(r.tm);
}

// world->hit for `r` (main.cu:57) begins: nothing hit under tmax, the ray's box-test terms, the root
DEV void walk_start(const Ray& r, const float* bound, float tmax, HitInfo& best, f3& inv, bool& loose, LooseRay& lr, int& node) {
    best.t = tmax; best.prim = -1; best.inst = -1;
    inv = mk3(1.0f / r.d.x, 1.0f / r.d.y, 1.0f / r.d.z);
    loose = inv_is_finite(inv) && loose_ok(inv, r.o, bound);
    lr = loose_setup(inv, r.o, bound);
    node = 0;
}

// One node visit of the walk for a ray with the window (tmin, best.t): bvh_node::hit (bvh.cuh:95-106) as trace() walks it,
// with the render kernels' guards on the faster box tests.  `loose` (every 1/d component finite and loose_ok): interior
// boxes take the widened one-fma form, a superset of aabb::hit's passes, and a leaf's own box is tested again exactly
// (slab_test_finite) before its object -- the walk then reaches exactly the objects the reference reaches (rt_device_funcs.h,
// "the walk loop's box test").  Otherwise (a zero direction component): the reference's own
// slab form everywhere.  Returns the next node; for ANY it returns n_nodes at the first accepted leaf.
template <bool SPHERES_ONLY, bool ANY>
DEV int walk_step(const SceneView& sc, const float4* nodes4, int node, const Ray& r, const f3 inv, const LooseRay& lr, bool loose,
                  float tmin, HitInfo& best) {
    const float4 a = nodes4[2 * node], b = nodes4[2 * node + 1];
    const bool pass = loose ? slab_test_loose(a, b, inv, lr, tmin, best.t) : slab_test(a, b, r.o, inv, tmin, best.t);
    // device encoding of the links (rt_device.h, RT_NODE_SKIP): a.w = ~skip; b.w = ~(node + 1) inside, the object id at a leaf
    const int32_t link = __float_as_int(b.w), nskip = __float_as_int(a.w);
    const bool is_leaf = link >= 0, inner = lane_not(is_leaf);   // compared once: the complement is mask logic
    int next = ~((pass && inner) ? link : nskip);
    if (pass && is_leaf && (!loose || slab_test_finite(a, b, r.o, inv, tmin, best.t))) {
        leaf_test<SPHERES_ONLY>(sc, link, r, tmin, best);
        if (ANY && best.prim >= 0) next = sc.n_nodes;
    }
    return next;
}

// p[0..2] = k v: a feature pass's store of a sum over ns samples
DEV void st3(float* p, f3 v, float k) { p[0] = v.x * k; p[1] = v.y * k; p[2] = v.z * k; }

}  // namespace
