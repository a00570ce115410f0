// rt_refit_host.h -- the host half of rt_scene_update_spheres, rt_scene_update_instances and rt_scene_update_quads
// (include/rt_abi.h): the box rules, the checks of an update and the refit of a node array in the
// description's link encoding.  Plain C++ with no HIP call, so that rt_refit_nodes needs no device and the same text compiles
// into a stand-alone host program; rt_kernel_refit.hip takes the box rules and the question "does this leaf follow a replaced
// record?" from here too, so host and device cannot drift apart.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/rt_abi.h"

#if defined(__HIPCC__)
#define RT_REFIT_HD __host__ __device__
#else
#define RT_REFIT_HD
#endif

namespace rt_refit {

// The kinds of record an update replaces.  One path serves all three (the checks below, refit_nodes, the kernels of
// rt_kernel_refit.hip, update_records of rt_abi.hip); what differs per kind is what a record must satisfy, what is stored beside
// it, and which leaves follow it (depends_on).
enum kind { SPHERES, INSTANCES, QUADS, KINDS };
struct noun { const char *one, *a_one, *many; };
static const noun NOUNS[KINDS] = {{"sphere", "a sphere", "spheres"}, {"instance", "an instance", "instances"}, {"quad", "a quad", "quads"}};
inline const rt_sphere* records_of(const rt_sphere_update& u) { return u.spheres; }
inline const rt_instance* records_of(const rt_instance_update& u) { return u.instances; }
inline const rt_quad* records_of(const rt_quad_update& u) { return u.quads; }

// The box rule (rt_abi.h): r = |radius|, a = c0 + 0 vel, b = c0 + 1 vel, lo = min(a - r, b - r), hi = max(a + r, b + r), every
// operation a binary32 one rounded once (the build has contraction off; a contracted form would round the same: 0 vel and
// 1 vel are exact).  For radius >= 0 this is the host library's sphere constructors value for value (host/rtw.cpp).
RT_REFIT_HD inline void sphere_box(const rt_sphere& s, float lo[3], float hi[3]) {
    const float r = fabsf(s.radius);
    for (int c = 0; c < 3; ++c) {
        const float a = s.c0[c] + 0.0f * s.vel[c];
        const float b = s.c0[c] + 1.0f * s.vel[c];
        lo[c] = fminf(a - r, b - r);
        hi[c] = fmaxf(a + r, b + r);
    }
}

// what the checks allow of a record: every float finite, mat one of the scene's materials
RT_REFIT_HD inline bool record_ok(const rt_sphere& s, int32_t n_materials) {
    // (x - x == 0 exactly for finite x only; written without isfinite so that host and device share the text)
    bool finite = s.radius - s.radius == 0.0f;
    for (int c = 0; c < 3; ++c) finite = finite && (s.c0[c] - s.c0[c] == 0.0f) && (s.vel[c] - s.vel[c] == 0.0f);
    return finite && s.mat >= 0 && s.mat < n_materials;
}

// per sphere: whether it is the child of an instance (its box then follows the instance's rule, which an update does not redo)
inline std::vector<char> instanced_spheres(const rt_instance* instances, int32_t n_instances, int32_t n_spheres) {
    std::vector<char> under((size_t)(n_spheres > 0 ? n_spheres : 0), 0);
    for (int i = 0; i < n_instances; ++i) {
        const int32_t c = instances[i].child;
        if (c >= 0 && RT_PRIM_KIND(c) == RT_PRIM_SPHERE && RT_PRIM_INDEX(c) < n_spheres) under[(size_t)RT_PRIM_INDEX(c)] = 1;
    }
    return under;
}

// The refusals every kind of update shares (rt_abi.h), none of which needs a device: null or empty text = fine.  n: the scene's
// count of the kind.  per_record(record, i) is asked about record k, which replaces record i of the scene, as soon as index k
// has passed -- before index k + 1 is looked at -- and answers with the refusal's text or null (no string is built per record:
// an update may carry every record of a large scene).
template <class Update, class PerRecord>
inline std::string check_indices(const Update* u, const noun& w, int32_t n, PerRecord&& per_record) {
    if (!u) return "null update";
    if (u->count < 0) return "count is negative";
    if (u->count == 0) return "";
    if (!records_of(*u)) return std::string("null ") + w.one + " records";
    if (u->count > n) return std::string("more records than the scene has ") + w.many + " (an index is out of range or appears twice)";
    std::vector<char> seen((size_t)n, 0);
    for (int32_t k = 0; k < u->count; ++k) {
        const long long i = u->indices ? (long long)u->indices[k] : (long long)u->first + k;
        if (i < 0 || i >= n) return std::string(w.one) + " index out of range";
        if (seen[(size_t)i]) return std::string(w.a_one) + " index appears twice";
        seen[(size_t)i] = 1;
        if (const char* why = per_record(records_of(*u)[k], (int32_t)i)) return why;
    }
    return "";
}

// The refusals of a sphere update.  host_records: the records can be read here (their values are checked); device-resident
// records are checked by the records kernel instead.
inline std::string check_update(const rt_sphere_update* u, bool host_records, int32_t n_spheres, int32_t n_materials,
                                const std::vector<char>& instanced) {
    const char* under = instanced.data();
    return check_indices(u, NOUNS[SPHERES], n_spheres, [=](const rt_sphere& s, int32_t i) -> const char* {
        if (under[i]) return "an updated sphere is the child of an instance (its box follows the instance's rule)";
        if (!host_records) return nullptr;
        const rt_sphere geometry = {{s.c0[0], s.c0[1], s.c0[2]}, s.radius, {s.vel[0], s.vel[1], s.vel[2]}, 0};
        if (!record_ok(geometry, 1)) return "a sphere record has a non-finite c0, vel or radius";
        if (s.mat < 0 || s.mat >= n_materials) return "sphere material out of range";
        return nullptr;
    });
}

// ---- instances (rt_scene_update_instances).  The rule is the host library's constructors restated operation by
// operation (host/rtw.cpp: quad::quad, compound6, rotate_y::rotate_y; rtw.h: translate), every operation a binary32 one rounded
// once; the only fused operations are the two fmaf of the rotation, which the constructor writes the same way.

// quad::quad: the padded union of the two diagonals' boxes
RT_REFIT_HD inline void quad_box(const rt_quad& q, float lo[3], float hi[3]) {
    for (int c = 0; c < 3; ++c) {
        const float a = q.Q[c] + q.u[c], b = q.Q[c] + q.v[c], p = a + q.v[c];
        lo[c] = fminf(fminf(q.Q[c], p), fminf(a, b)) - 1e-3f;
        hi[c] = fmaxf(fmaxf(q.Q[c], p), fmaxf(a, b)) + 1e-3f;
    }
}

// compound6: the six faces' boxes in array order.  first_quad's high bits are the device's marks (rt_scene_create) and masked off.
RT_REFIT_HD inline void box_box(const rt_box& b, const rt_quad* quads, float lo[3], float hi[3]) {
    const int32_t first = b.first_quad & 0x3FFFFFFF;   // (RT_BOX_FIRST_MASK, below)
    quad_box(quads[first], lo, hi);
    for (int f = 1; f < 6; ++f) {
        float l[3], h[3];
        quad_box(quads[first + f], l, h);
        for (int c = 0; c < 3; ++c) { lo[c] = fminf(lo[c], l[c]); hi[c] = fmaxf(hi[c], h[c]); }
    }
}

// The box of an instance's child in object space.  `child` is a reference rt_scene_create has validated: a sphere, quad or box
// inside its array (a box's six quads inside theirs).  Anything else -- which validation excludes -- reads nothing.
RT_REFIT_HD inline void child_box(int32_t child, const rt_sphere* spheres, const rt_quad* quads, const rt_box* boxes, float lo[3], float hi[3]) {
    const int kind = child < 0 ? -1 : (int)RT_PRIM_KIND(child), i = (int)RT_PRIM_INDEX(child);
    if (kind == RT_PRIM_SPHERE) sphere_box(spheres[i], lo, hi);
    else if (kind == RT_PRIM_QUAD) quad_box(quads[i], lo, hi);
    else if (kind == RT_PRIM_BOX) box_box(boxes[i], quads, lo, hi);
    else for (int c = 0; c < 3; ++c) { lo[c] = 0.0f; hi[c] = 0.0f; }
}

// translate(rotate_y(child box)): the eight corners in the constructor's order (x outer, z inner), then the offset
RT_REFIT_HD inline void instance_box(const rt_instance& in, float lo[3], float hi[3]) {
    if (in.flags & RT_INST_ROTATE_Y) {
        float l[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, h[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
        for (int i = 0; i < 2; ++i)
            for (int j = 0; j < 2; ++j)
                for (int k = 0; k < 2; ++k) {
                    const float x = i ? hi[0] : lo[0], y = j ? hi[1] : lo[1], z = k ? hi[2] : lo[2];
                    const float r[3] = {fmaf(in.cos_t, x, in.sin_t * z), y, fmaf(in.cos_t, z, -(in.sin_t * x))};
                    for (int c = 0; c < 3; ++c) { l[c] = fminf(l[c], r[c]); h[c] = fmaxf(h[c], r[c]); }
                }
        for (int c = 0; c < 3; ++c) { lo[c] = l[c]; hi[c] = h[c]; }
    }
    if (in.flags & RT_INST_TRANSLATE)
        for (int c = 0; c < 3; ++c) { lo[c] = lo[c] + in.offset[c]; hi[c] = hi[c] + in.offset[c]; }
}

// what the checks allow of an instance record: sin_t, cos_t and offset finite, flags 1, 2 or 3, child the scene's own
RT_REFIT_HD inline bool instance_finite(const rt_instance& in) {
    bool finite = (in.sin_t - in.sin_t == 0.0f) && (in.cos_t - in.cos_t == 0.0f);
    for (int c = 0; c < 3; ++c) finite = finite && (in.offset[c] - in.offset[c] == 0.0f);
    return finite;
}
RT_REFIT_HD inline bool instance_record_ok(const rt_instance& in, int32_t scene_child) {
    return instance_finite(in) && in.flags >= 1 && in.flags <= 3 && in.child == scene_child;
}

// The refusals of an instance update (rt_abi.h), as check_update.  children: per instance, the child the scene holds.
inline std::string check_instance_update(const rt_instance_update* u, bool host_records, const int32_t* children, int32_t n_instances) {
    const std::string why = check_indices(u, NOUNS[INSTANCES], n_instances, [](const rt_instance&, int32_t) -> const char* { return nullptr; });
    if (!why.empty() || !u || u->count <= 0 || !host_records) return why;
    for (int32_t k = 0; k < u->count; ++k) {   // (after every index has passed: a record is compared with the instance it names)
        const int32_t i = u->indices ? u->indices[k] : u->first + k;
        const rt_instance& in = u->instances[k];
        if (!instance_finite(in)) return "an instance record has a non-finite sin_t, cos_t or offset";
        if (in.flags < 1 || in.flags > 3) return "instance flags must be 1, 2 or 3";
        if (in.child != children[(size_t)i]) return "an instance record's child is not the child the scene holds (the child of an instance cannot change)";
    }
    return "";
}

// Refit of a node array in the description's encoding (skip = index of the next node when the box is missed, prim < 0 =
// interior, depth-first pre-order): leaf_rule(prim, bmin, bmax) is called for every leaf and rewrites the box of those it
// recomputes, then every interior node becomes the float min / max union of its children's boxes, children before parents (a
// node's children are i + 1 and the nodes its skip chain reaches below skip[i]).  Link words are not written.
template <class LeafRule>
inline void refit_nodes(rt_node* nodes, int32_t n, LeafRule&& leaf_rule) {
    for (int32_t i = 0; i < n; ++i)
        if (nodes[i].prim >= 0) leaf_rule(nodes[i].prim, nodes[i].bmin, nodes[i].bmax);
    for (int32_t i = n - 1; i >= 0; --i) {
        if (nodes[i].prim >= 0) continue;
        bool first = true;
        for (int32_t j = i + 1; j < nodes[i].skip && j < n; j = nodes[j].skip) {
            for (int c = 0; c < 3; ++c) {
                nodes[i].bmin[c] = first ? nodes[j].bmin[c] : fminf(nodes[i].bmin[c], nodes[j].bmin[c]);
                nodes[i].bmax[c] = first ? nodes[j].bmax[c] : fmaxf(nodes[i].bmax[c], nodes[j].bmax[c]);
            }
            first = false;
        }
    }
}

// ---- quads and boxes (rt_scene_update_quads).  The boxes are quad_box / box_box / child_box / instance_box above;
// what is new is the data rt_scene_create derives from quad records and keeps on the device -- the axis code in rt_quad.pad0 and
// the canonical-box mark, bit 30 of rt_box.first_quad (quad_test_axis and the six-face fast path, rt_device_funcs.h) --, which
// creation and update take from the same two functions here.

// The axis of an axis-aligned quad, or -1: its unit normal is exactly +-e_C and u, v, w each have exactly one non-zero component
// on the fitting axes.
RT_REFIT_HD inline int axis_of(const rt_quad& q) {
    for (int c = 0; c < 3; ++c) {
        const int a = (c + 1) % 3, b = (c + 2) % 3;
        if (!((q.n[c] == 1.0f || q.n[c] == -1.0f) && q.n[a] == 0.0f && q.n[b] == 0.0f)) continue;
        if (!(q.w[a] == 0.0f && q.w[b] == 0.0f && q.w[c] != 0.0f && q.u[c] == 0.0f && q.v[c] == 0.0f)) continue;
        const bool u_on_a = q.u[a] != 0.0f && q.u[b] == 0.0f, u_on_b = q.u[b] != 0.0f && q.u[a] == 0.0f;
        const bool v_on_a = q.v[a] != 0.0f && q.v[b] == 0.0f, v_on_b = q.v[b] != 0.0f && q.v[a] == 0.0f;
        if ((u_on_a && v_on_b) || (u_on_b && v_on_a)) return c;
    }
    return -1;
}
// the word rt_quad.pad0 holds on the device: 1 + axis, 0 for any other quad
RT_REFIT_HD inline int32_t axis_code(const rt_quad& q) { const int c = axis_of(q); return c >= 0 ? 1 + c : 0; }
#define RT_BOX_CANONICAL 0x40000000
#define RT_BOX_FIRST_MASK 0x3FFFFFFF
// A box is canonical when its six faces are axis-aligned with normals along z, x, z, x, y, y (make_box's order, the reference's
// quad.cuh:145-162): codes[f] is the axis code of face f.
RT_REFIT_HD inline bool canonical_codes(const int32_t codes[6]) {
    return codes[0] == 3 && codes[1] == 1 && codes[2] == 3 && codes[3] == 1 && codes[4] == 2 && codes[5] == 2;
}

// what the checks allow of a quad record: Q, D, u, v, w, n finite, mat one of the scene's materials (pad0..2 are not looked at)
RT_REFIT_HD inline bool quad_finite(const rt_quad& q) {
    bool finite = q.D - q.D == 0.0f;
    for (int c = 0; c < 3; ++c)
        finite = finite && (q.Q[c] - q.Q[c] == 0.0f) && (q.u[c] - q.u[c] == 0.0f) && (q.v[c] - q.v[c] == 0.0f) && (q.w[c] - q.w[c] == 0.0f) &&
                 (q.n[c] - q.n[c] == 0.0f);
    return finite;
}
RT_REFIT_HD inline bool quad_record_ok(const rt_quad& q, int32_t n_materials) { return quad_finite(q) && q.mat >= 0 && q.mat < n_materials; }

// The solid a leaf's box follows: the leaf's primitive, or the boundary of the leaf's constant_medium -- a reference to a sphere,
// quad, box or instance inside its array, or -1.
inline int32_t leaf_solid(int32_t prim, const rt_medium* media, int32_t n_media, int32_t n_spheres, int32_t n_quads, int32_t n_boxes, int32_t n_instances) {
    if (prim < 0) return -1;
    if (RT_PRIM_KIND(prim) == RT_PRIM_MEDIUM) {
        const int m = RT_PRIM_INDEX(prim);
        if (m >= n_media) return -1;
        prim = media[m].boundary;
        if (prim < 0) return -1;
    }
    const int kind = RT_PRIM_KIND(prim), i = RT_PRIM_INDEX(prim);
    const int32_t n = kind == RT_PRIM_SPHERE ? n_spheres : kind == RT_PRIM_QUAD ? n_quads : kind == RT_PRIM_BOX ? n_boxes : kind == RT_PRIM_INSTANCE ? n_instances : 0;
    return i < n ? prim : -1;
}

// Whether a solid depends on a quad for which moved(i) holds: a quad by itself, a box by any of its six faces, an instance by the
// same test of its stored child.  Every reference is one rt_scene_create has validated (or leaf_solid has bounded).
template <class Moved>
RT_REFIT_HD inline bool solid_moved(int32_t solid, const rt_box* boxes, const rt_instance* instances, Moved&& moved) {
    if (solid < 0) return false;
    if (RT_PRIM_KIND(solid) == RT_PRIM_INSTANCE) solid = instances[RT_PRIM_INDEX(solid)].child;
    if (solid < 0) return false;
    const int kind = RT_PRIM_KIND(solid), i = RT_PRIM_INDEX(solid);
    if (kind == RT_PRIM_QUAD) return moved(i);
    if (kind != RT_PRIM_BOX) return false;
    const int32_t first = boxes[i].first_quad & RT_BOX_FIRST_MASK;
    bool any = false;
    for (int f = 0; f < 6; ++f) any = any || moved(first + f);
    return any;
}
// Whether a solid depends on a record of `kind` for which moved(i) holds.  A sphere update moves the solid that is that sphere
// and never looks through an instance (check_update refuses an instanced sphere: its box follows the instance's rule); an
// instance update moves the solid that is that instance; a quad update moves what solid_moved says.
template <class Moved>
RT_REFIT_HD inline bool depends_on(int kind, int32_t solid, const rt_box* boxes, const rt_instance* instances, Moved&& moved) {
    if (kind == QUADS) return solid_moved(solid, boxes, instances, moved);
    return solid >= 0 && (int)RT_PRIM_KIND(solid) == (kind == SPHERES ? RT_PRIM_SPHERE : RT_PRIM_INSTANCE) && moved((int)RT_PRIM_INDEX(solid));
}
// the box of a solid by the rules of rt_abi.h: the sphere, quad and box rules, and the instance rule over its child's box
RT_REFIT_HD inline void solid_box(int32_t solid, const rt_sphere* spheres, const rt_quad* quads, const rt_box* boxes, const rt_instance* instances,
                                  float lo[3], float hi[3]) {
    if (RT_PRIM_KIND(solid) == RT_PRIM_INSTANCE) {
        const rt_instance in = instances[RT_PRIM_INDEX(solid)];
        child_box(in.child, spheres, quads, boxes, lo, hi);
        instance_box(in, lo, hi);
    } else child_box(solid, spheres, quads, boxes, lo, hi);
}

// The refusals of a quad update (rt_abi.h), as check_update.
inline std::string check_quad_update(const rt_quad_update* u, bool host_records, int32_t n_quads, int32_t n_materials) {
    return check_indices(u, NOUNS[QUADS], n_quads, [=](const rt_quad& q, int32_t) -> const char* {
        if (!host_records) return nullptr;
        if (!quad_finite(q)) return "a quad record has a non-finite Q, D, u, v, w or n";
        if (q.mat < 0 || q.mat >= n_materials) return "quad material out of range";
        return nullptr;
    });
}

// The leaves whose solid depends on a record of `kind` marked in `moved` take their rule's box over spheres[...], instances[...]
// and quads[...]: the arrays of the description `d`, whose references rt_scene_create's checks have validated, with the update's
// records in place.
inline void refit_nodes(rt_node* nodes, const rt_scene_desc* d, const rt_sphere* spheres, const rt_instance* instances, const rt_quad* quads,
                        int kind, const std::vector<char>& moved) {
    refit_nodes(nodes, d->n_nodes, [&](int32_t prim, float* lo, float* hi) {
        const int32_t solid = leaf_solid(prim, d->media, d->n_media, d->n_spheres, d->n_quads, d->n_boxes, d->n_instances);
        if (!depends_on(kind, solid, d->boxes, instances, [&](int i) { return moved[(size_t)i] != 0; })) return;
        solid_box(solid, spheres, quads, d->boxes, instances, lo, hi);
    });
}

}  // namespace rt_refit
